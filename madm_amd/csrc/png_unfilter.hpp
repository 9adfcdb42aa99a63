// PNG scanline unfiltering (PNG specification, section 9: filter types 0 .. 4), plain host C++ with no dependency: data.hip
// exports it as mdata_png_unfilter, tools/png_unfilter_check.cpp compiles it alone under the host sanitizers.
// Every index is derived from (height, row_bytes, bpp) after the two lengths were checked against them, never from the data.
#pragma once
#include <stddef.h>
#include <stdint.h>

// 0 = ok, 1 = inconsistent arguments (nothing touched), 3 = bad filter byte; *bad_row (if given) = the offending row
static inline int png_unfilter_rows(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_len, int height,
                                    size_t row_bytes, int bpp, int* bad_row) {
    if (!in || !out || height <= 0 || row_bytes == 0 || bpp < 1 || bpp > 8) return 1;
    const size_t h = (size_t)height;
    if (row_bytes > (SIZE_MAX / h) - 1) return 1;                       // h * (1 + row_bytes) must not wrap
    if (in_len != h * (1 + row_bytes) || out_len != h * row_bytes) return 1;
    const size_t b = (size_t)bpp;
    const size_t head = b < row_bytes ? b : row_bytes;                  // bytes of a row without a left neighbour
    for (size_t y = 0; y < h; ++y) {
        const uint8_t* s = in + y * (1 + row_bytes);
        const unsigned f = s[0];
        if (f > 4) {
            if (bad_row) *bad_row = (int)y;
            return 3;
        }
        ++s;
        uint8_t* d = out + y * row_bytes;
        const uint8_t* up = y ? d - row_bytes : nullptr;                // the row above, already decoded; none above row 0
        switch (f) {
        case 0:
            for (size_t i = 0; i < row_bytes; ++i) d[i] = s[i];
            break;
        case 1:
            for (size_t i = 0; i < head; ++i) d[i] = s[i];
            for (size_t i = head; i < row_bytes; ++i) d[i] = (uint8_t)(s[i] + d[i - b]);
            break;
        case 2:
            for (size_t i = 0; i < row_bytes; ++i) d[i] = (uint8_t)(s[i] + (up ? up[i] : 0));
            break;
        case 3:
            for (size_t i = 0; i < head; ++i) d[i] = (uint8_t)(s[i] + ((up ? up[i] : 0) >> 1));
            for (size_t i = head; i < row_bytes; ++i) d[i] = (uint8_t)(s[i] + (((unsigned)d[i - b] + (up ? up[i] : 0u)) >> 1));
            break;
        default:   // 4, Paeth: with no left and no upper-left neighbour the predictor is the byte above
            for (size_t i = 0; i < head; ++i) d[i] = (uint8_t)(s[i] + (up ? up[i] : 0));
            for (size_t i = head; i < row_bytes; ++i) {
                const int a = d[i - b], bb = up ? up[i] : 0, c = up ? up[i - b] : 0;
                const int p = a + bb - c;
                const int pa = p > a ? p - a : a - p, pb = p > bb ? p - bb : bb - p, pc = p > c ? p - c : c - p;
                const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? bb : c);
                d[i] = (uint8_t)(s[i] + pred);
            }
            break;
        }
    }
    return 0;
}
