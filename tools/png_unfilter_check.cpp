// Host-sanitizer check of the PNG reader's native part (madm_amd/csrc/png_unfilter.hpp, exported by libmadm_data.so as
// mdata_png_unfilter).  A stand-alone CPU program; build and run it with the host sanitizers:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Imadm_amd/csrc \
//       tools/png_unfilter_check.cpp -o /tmp/png_unfilter_check && /tmp/png_unfilter_check
//
// Every buffer is a heap allocation of exactly the stated size, so one byte read or written past an end is reported.
// It feeds valid rows of every filter type (checked against a forward filter written here), every bpp 1 .. 8, rows shorter
// than one pixel, and malformed input: random filter bytes, bad lengths, null pointers.  Prints "ok" and returns 0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "png_unfilter.hpp"

static unsigned rng_state = 12345u;
static unsigned rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return rng_state >> 8;
}

static int paeth(int a, int b, int c) {
    const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

// forward filter of raw rows (the PNG specification's definition, from the raw bytes)
static void filter_forward(const uint8_t* raw, uint8_t* out, int h, size_t n, int bpp, const uint8_t* types) {
    for (int y = 0; y < h; ++y) {
        const uint8_t* r = raw + (size_t)y * n;
        const uint8_t* u = y ? r - n : nullptr;
        uint8_t* o = out + (size_t)y * (n + 1);
        o[0] = types[y];
        for (size_t i = 0; i < n; ++i) {
            const int a = i >= (size_t)bpp ? r[i - bpp] : 0, b = u ? u[i] : 0, c = (u && i >= (size_t)bpp) ? u[i - bpp] : 0;
            int pred = 0;
            switch (types[y]) {
            case 1: pred = a; break;
            case 2: pred = b; break;
            case 3: pred = (a + b) >> 1; break;
            case 4: pred = paeth(a, b, c); break;
            default: pred = 0; break;
            }
            o[1 + i] = (uint8_t)(r[i] - pred);
        }
    }
}

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                      \
        }                                                                  \
    } while (0)

int main() {
    long cases = 0;
    for (int bpp = 1; bpp <= 8; ++bpp) {
        for (int h = 1; h <= 5; ++h) {
            for (size_t n = 1; n <= 19; n += (n < 9 ? 1 : 5)) {
                for (int mode = 0; mode < 7; ++mode) {      // 0 .. 4: one type; 5: mixed valid; 6: a bad filter byte somewhere
                    std::vector<uint8_t> raw((size_t)h * n), types((size_t)h);
                    for (auto& v : raw) v = (rnd() & 3) ? (uint8_t)rnd() : (uint8_t)7;
                    for (auto& t : types) t = (uint8_t)(mode < 5 ? mode : rnd() % 5);
                    const int bad = mode == 6 ? (int)(rnd() % (unsigned)h) : -1;
                    uint8_t* in = (uint8_t*)malloc((size_t)h * (n + 1));
                    uint8_t* out = (uint8_t*)malloc((size_t)h * n);
                    CHECK(in && out);
                    filter_forward(raw.data(), in, h, n, bpp, types.data());
                    if (bad >= 0) in[(size_t)bad * (n + 1)] = (uint8_t)(5 + rnd() % 251);
                    memset(out, 0xA5, (size_t)h * n);
                    int bad_row = -1;
                    const int rc = png_unfilter_rows(in, (size_t)h * (n + 1), out, (size_t)h * n, h, n, bpp, &bad_row);
                    if (bad < 0) {
                        CHECK(rc == 0);
                        CHECK(memcmp(out, raw.data(), (size_t)h * n) == 0);
                    } else {
                        CHECK(rc == 3 && bad_row == bad);
                        CHECK(memcmp(out, raw.data(), (size_t)bad * n) == 0);
                        for (size_t i = (size_t)bad * n; i < (size_t)h * n; ++i) CHECK(out[i] == 0xA5);
                    }
                    // inconsistent arguments: refused before any access (the buffers are really that much shorter)
                    uint8_t* in_short = (uint8_t*)malloc((size_t)h * (n + 1) - 1);
                    CHECK(in_short);
                    CHECK(png_unfilter_rows(in_short, (size_t)h * (n + 1) - 1, out, (size_t)h * n, h, n, bpp, nullptr) == 1);
                    CHECK(png_unfilter_rows(in, (size_t)h * (n + 1), out, (size_t)h * n - 1, h, n, bpp, nullptr) == 1);
                    CHECK(png_unfilter_rows(in, (size_t)h * (n + 1), out, (size_t)h * n, h + 1, n, bpp, nullptr) == 1);
                    CHECK(png_unfilter_rows(in, (size_t)h * (n + 1), out, (size_t)h * n, h, n + 1, bpp, nullptr) == 1);
                    CHECK(png_unfilter_rows(in, (size_t)h * (n + 1), out, (size_t)h * n, h, n, 0, nullptr) == 1);
                    CHECK(png_unfilter_rows(in, (size_t)h * (n + 1), out, (size_t)h * n, h, n, 9, nullptr) == 1);
                    CHECK(png_unfilter_rows(in, (size_t)h * (n + 1), out, (size_t)h * n, -h, n, bpp, nullptr) == 1);
                    CHECK(png_unfilter_rows(nullptr, (size_t)h * (n + 1), out, (size_t)h * n, h, n, bpp, nullptr) == 1);
                    CHECK(png_unfilter_rows(in, (size_t)h * (n + 1), nullptr, (size_t)h * n, h, n, bpp, nullptr) == 1);
                    free(in_short);
                    free(in);
                    free(out);
                    ++cases;
                }
            }
        }
    }
    // sizes whose product wraps size_t
    uint8_t one[2] = {0, 0};
    CHECK(png_unfilter_rows(one, 2, one, 1, 2147483647, SIZE_MAX / 2, 1, nullptr) == 1);
    CHECK(png_unfilter_rows(one, 0, one, 0, 2, SIZE_MAX, 1, nullptr) == 1);
    // random garbage as scanlines: any status, no out-of-bounds access
    for (int t = 0; t < 2000; ++t) {
        const int h = 1 + (int)(rnd() % 6), bpp = 1 + (int)(rnd() % 8);
        const size_t n = 1 + rnd() % 24;
        uint8_t* in = (uint8_t*)malloc((size_t)h * (n + 1));
        uint8_t* out = (uint8_t*)malloc((size_t)h * n);
        CHECK(in && out);
        for (size_t i = 0; i < (size_t)h * (n + 1); ++i) in[i] = (uint8_t)rnd();
        for (int y = 0; y < h; ++y)
            if (rnd() & 1) in[(size_t)y * (n + 1)] = (uint8_t)(rnd() % 6);
        const int rc = png_unfilter_rows(in, (size_t)h * (n + 1), out, (size_t)h * n, h, n, bpp, nullptr);
        CHECK(rc == 0 || rc == 3);
        free(in);
        free(out);
        ++cases;
    }
    printf("png_unfilter_check: %ld cases ok\n", cases);
    return 0;
}
