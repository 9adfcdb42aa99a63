// libmadm_data.so (include/madm_data.h): the dataset pipeline's two kernels and the PNG reader's unfilter loop.
//
// mdata_prep_image_u8: the reference's load_aug_data for a 'data' file (data/dataset/cross_modality_dataset.py:352-381) in
// one launch -- PIL's two-pass fixed-point BILINEAR resize, crop, flip, channel repeat and float cast, computed for the crop
// only.  One workgroup owns a TY x TX tile of the crop: it runs the horizontal pass for the source rows of the tile's
// vertical footprint (at most TY * 8 + MAX_TAPS + 1 rows: scale factors above 8 are refused) into LDS as uint8, exactly the
// intermediate image PIL keeps, then the vertical pass reads LDS and stores three planes, consecutive lanes consecutive x.
// mdata_prep_label_u8: the 'label' file -- NEAREST gather through two index tables, crop, flip, the DELIVER rule and
// label_convert as two 256-entry tables, and the 256-bin histogram rare-class sampling counts.
// Both are byte traffic far off the critical path (a 512 x 512 crop is 3 MB of stores); nothing here is tuned.
//
// Memory safety does not depend on the tables' contents: every window is clamped to the source, every tap count to the
// table width and to the footprint held in LDS.
#include "entry.hpp"
#include "madm_data.h"
#include "png_unfilter.hpp"

namespace {

#define MDATA_REQUIRE(...) ENTRY_REQUIRE(MDATA_ERR_INVALID_ARG, __VA_ARGS__)

constexpr int TY = 16, TX = 64;                           // crop pixels per workgroup (256 threads, 4 rows each)
constexpr int FOOT = TY * 8 + MDATA_MAX_TAPS + 1;         // source rows a tile's vertical pass can touch at scale <= 8

struct ImageGeom {
    int C, src_ld, in_h, in_w, hk, vk, y0, x0, ch, cw, flip, out_ld, out_plane;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// Unsigned accumulation: the recipe's coefficients are non-negative and a row's sum stays below 2^30 + 2^21, where this equals
// Pillow's signed arithmetic; a table from elsewhere wraps modulo 2^32 (other pixels, never undefined behaviour).
__device__ __forceinline__ unsigned clip8(unsigned acc) { return min((acc + (1u << 21)) >> 22, 255u); }

__global__ __launch_bounds__(256) void prep_image_kernel(const ImageGeom g, const uint8_t* __restrict__ src,
                                                         const int32_t* __restrict__ hbounds,
                                                         const int32_t* __restrict__ hcoef,
                                                         const int32_t* __restrict__ vbounds,
                                                         const int32_t* __restrict__ vcoef, float* __restrict__ out) {
    __shared__ uint8_t s_h[FOOT * 3 * TX];                // [footprint row][channel][tile column]
    __shared__ int s_ymin[TY], s_n[TY];
    const int tid = threadIdx.x;
    const int cx0 = blockIdx.x * TX, cy0 = blockIdx.y * TY;
    const int ncols = min(TX, g.cw - cx0), nrows = min(TY, g.ch - cy0);

    // the tile rows' windows into the source, clamped to it
    if (tid < TY) {
        int ymin = 0, n = 0;
        if (tid < nrows) {
            const int ry = g.y0 + cy0 + tid;
            if (vbounds) {
                ymin = clampi(vbounds[2 * ry], 0, g.in_h - 1);
                n = clampi(vbounds[2 * ry + 1], 0, min(g.vk, g.in_h - ymin));
            } else {
                ymin = ry;                                 // pass skipped: rh == in_h
                n = 1;
            }
        }
        s_ymin[tid] = ymin;
        s_n[tid] = n;
    }
    __syncthreads();
    int f0 = s_ymin[0], f1 = s_ymin[0] + s_n[0];
    for (int r = 1; r < nrows; ++r) {
        f0 = min(f0, s_ymin[r]);
        f1 = max(f1, s_ymin[r] + s_n[r]);
    }
    const int nf = min(f1 - f0, FOOT);

    // horizontal pass: footprint rows x tile columns -> LDS, uint8
    for (int idx = tid; idx < nf * ncols; idx += 256) {
        const int fr = idx / ncols, c = idx - fr * ncols;
        const int rx = g.x0 + cx0 + c;
        const uint8_t* row = src + (size_t)(f0 + fr) * (size_t)g.src_ld;
        uint8_t* dst = s_h + fr * (3 * TX) + c;
        if (hbounds) {
            const int xmin = clampi(hbounds[2 * rx], 0, g.in_w - 1);
            const int n = clampi(hbounds[2 * rx + 1], 0, min(g.hk, g.in_w - xmin));
            const int32_t* k = hcoef + (size_t)rx * g.hk;
            if (g.C == 3) {
                unsigned a0 = 0, a1 = 0, a2 = 0;
                const uint8_t* p = row + 3 * xmin;
                for (int t = 0; t < n; ++t) {
                    const unsigned w = (unsigned)k[t];
                    a0 += (unsigned)p[3 * t] * w;
                    a1 += (unsigned)p[3 * t + 1] * w;
                    a2 += (unsigned)p[3 * t + 2] * w;
                }
                dst[0] = (uint8_t)clip8(a0);
                dst[TX] = (uint8_t)clip8(a1);
                dst[2 * TX] = (uint8_t)clip8(a2);
            } else {
                unsigned a0 = 0;
                const uint8_t* p = row + xmin;
                for (int t = 0; t < n; ++t) a0 += (unsigned)p[t] * (unsigned)k[t];
                dst[0] = (uint8_t)clip8(a0);
            }
        } else {                                           // pass skipped: rw == in_w
            if (g.C == 3) {
                dst[0] = row[3 * rx];
                dst[TX] = row[3 * rx + 1];
                dst[2 * TX] = row[3 * rx + 2];
            } else {
                dst[0] = row[rx];
            }
        }
    }
    __syncthreads();

    // vertical pass from LDS, planar stores (lane = column)
    const int c = tid & (TX - 1);
    if (c >= ncols) return;
    const int ox = g.flip ? g.cw - 1 - (cx0 + c) : cx0 + c;
    for (int r = tid / TX; r < nrows; r += 256 / TX) {
        const int fy = s_ymin[r] - f0;
        const int n = clampi(s_n[r], 0, nf - fy);          // nf < f1 - f0 only for tables the recipe cannot produce
        const uint8_t* p = s_h + fy * (3 * TX) + c;
        unsigned v0, v1, v2;
        if (vcoef) {
            const int32_t* k = vcoef + (size_t)(g.y0 + cy0 + r) * g.vk;
            if (g.C == 3) {
                unsigned a0 = 0, a1 = 0, a2 = 0;
                for (int t = 0; t < n; ++t) {
                    const unsigned w = (unsigned)k[t];
                    a0 += (unsigned)p[t * 3 * TX] * w;
                    a1 += (unsigned)p[t * 3 * TX + TX] * w;
                    a2 += (unsigned)p[t * 3 * TX + 2 * TX] * w;
                }
                v0 = clip8(a0); v1 = clip8(a1); v2 = clip8(a2);
            } else {
                unsigned a0 = 0;
                for (int t = 0; t < n; ++t) a0 += (unsigned)p[t * 3 * TX] * (unsigned)k[t];
                v0 = v1 = v2 = clip8(a0);
            }
        } else if (n > 0) {
            v0 = p[0];
            v1 = g.C == 3 ? p[TX] : v0;
            v2 = g.C == 3 ? p[2 * TX] : v0;
        } else {
            v0 = v1 = v2 = 0u;
        }
        float* o = out + (size_t)(cy0 + r) * (size_t)g.out_ld + ox;
        o[0] = (float)v0;
        o[(size_t)g.out_plane] = (float)v1;
        o[2 * (size_t)g.out_plane] = (float)v2;
    }
}

struct LabelGeom {
    int src_px, src_ld, in_h, in_w, y0, x0, ch, cw, flip, out_ld;
};

constexpr int LY = 4;                                      // label tile: LY x TX pixels, one per thread

__global__ __launch_bounds__(256) void prep_label_kernel(const LabelGeom g, const uint8_t* __restrict__ src,
                                                         const int32_t* __restrict__ ytab,
                                                         const int32_t* __restrict__ xtab,
                                                         const uint8_t* __restrict__ lut1,
                                                         const uint8_t* __restrict__ lut2, int32_t* __restrict__ hist,
                                                         int64_t* __restrict__ out) {
    __shared__ int s_hist[256];
    const int tid = threadIdx.x;
    if (hist) {
        s_hist[tid] = 0;
        __syncthreads();
    }
    const int cx = blockIdx.x * TX + (tid & (TX - 1));
    const int cy = blockIdx.y * LY + tid / TX;
    if (cx < g.cw && cy < g.ch) {
        const int ry = g.y0 + cy, rx = g.x0 + cx;
        const int sy = clampi(ytab ? ytab[ry] : ry, 0, g.in_h - 1);
        const int sx = clampi(xtab ? xtab[rx] : rx, 0, g.in_w - 1);
        unsigned v = src[(size_t)sy * (size_t)g.src_ld + (size_t)sx * (size_t)g.src_px];
        if (lut1) v = lut1[v];
        if (hist) atomicAdd(&s_hist[v], 1);
        if (lut2) v = lut2[v];
        const int ox = g.flip ? g.cw - 1 - cx : cx;
        out[(size_t)cy * (size_t)g.out_ld + ox] = (int64_t)v;
    }
    if (hist) {
        __syncthreads();
        const int n = s_hist[tid];
        if (n) atomicAdd(&hist[tid], n);
    }
}

}  // namespace

extern "C" int mdata_abi_version(void) { return 1; }

extern "C" const char* mdata_last_error(void) { return g_err; }

extern "C" int mdata_prep_image_u8(const uint8_t* src, int C, int src_ld, int in_h, int in_w, const int32_t* hbounds,
                                   const int32_t* hcoef, int hk, const int32_t* vbounds, const int32_t* vcoef, int vk,
                                   int rh, int rw, int y0, int x0, int ch, int cw, int flip, float* out, int out_ld,
                                   int out_plane, void* stream) {
    MDATA_REQUIRE(src && out, "prep_image_u8: null src or out");
    MDATA_REQUIRE(C == 1 || C == 3, "prep_image_u8: 1 or 3 interleaved channels, got %d", C);
    MDATA_REQUIRE(in_h > 0 && in_w > 0 && rh > 0 && rw > 0, "prep_image_u8: bad sizes in %d x %d -> %d x %d", in_h, in_w, rh, rw);
    MDATA_REQUIRE((long long)src_ld >= (long long)in_w * C, "prep_image_u8: src_ld %d bytes < in_w * C = %d", src_ld, in_w * C);
    MDATA_REQUIRE((long long)in_h * src_ld < 0x7fffffffLL, "prep_image_u8: source of %d rows x %d bytes is too large", in_h, src_ld);
    MDATA_REQUIRE(ch > 0 && cw > 0 && y0 >= 0 && x0 >= 0 && (long long)y0 + ch <= rh && (long long)x0 + cw <= rw,
                  "prep_image_u8: crop %d x %d at (%d, %d) leaves the %d x %d image", ch, cw, y0, x0, rh, rw);
    MDATA_REQUIRE((hbounds != nullptr) == (hcoef != nullptr) && (vbounds != nullptr) == (vcoef != nullptr),
                  "prep_image_u8: a pass needs both its bounds and its coefficients, or neither");
    if (hbounds) {
        MDATA_REQUIRE(hk >= 1 && hk <= MDATA_MAX_TAPS,
                      "prep_image_u8: %d horizontal taps (1 .. %d: scale factors above 8 are not supported)", hk, MDATA_MAX_TAPS);
        MDATA_REQUIRE((long long)in_w <= 8LL * rw, "prep_image_u8: width %d -> %d is a scale factor above 8", in_w, rw);
    } else {
        MDATA_REQUIRE(rw == in_w, "prep_image_u8: the horizontal pass can be skipped only when rw == in_w (%d vs %d)", rw, in_w);
        hk = 0;
    }
    if (vbounds) {
        MDATA_REQUIRE(vk >= 1 && vk <= MDATA_MAX_TAPS,
                      "prep_image_u8: %d vertical taps (1 .. %d: scale factors above 8 are not supported)", vk, MDATA_MAX_TAPS);
        MDATA_REQUIRE((long long)in_h <= 8LL * rh, "prep_image_u8: height %d -> %d is a scale factor above 8", in_h, rh);
    } else {
        MDATA_REQUIRE(rh == in_h, "prep_image_u8: the vertical pass can be skipped only when rh == in_h (%d vs %d)", rh, in_h);
        vk = 0;
    }
    MDATA_REQUIRE(aligned(hbounds, 4) && aligned(hcoef, 4) && aligned(vbounds, 4) && aligned(vcoef, 4),
                  "prep_image_u8: the tables must be 4-byte aligned");
    MDATA_REQUIRE(aligned(out, 4), "prep_image_u8: out must be 4-byte aligned");
    MDATA_REQUIRE(flip == 0 || flip == 1, "prep_image_u8: flip is 0 or 1, got %d", flip);
    MDATA_REQUIRE(out_ld >= cw && (long long)out_plane >= (long long)ch * out_ld,
                  "prep_image_u8: out_ld %d / out_plane %d too small for a %d x %d crop", out_ld, out_plane, ch, cw);
    const unsigned gx = (unsigned)((cw + TX - 1) / TX), gy = (unsigned)((ch + TY - 1) / TY);
    MDATA_REQUIRE(gy <= 65535u, "prep_image_u8: crop of %d rows is too tall", ch);
    ImageGeom g{C, src_ld, in_h, in_w, hk, vk, y0, x0, ch, cw, flip, out_ld, out_plane};
    prep_image_kernel<<<dim3(gx, gy), 256, 0, (hipStream_t)stream>>>(g, src, hbounds, hcoef, vbounds, vcoef, out);
    return check_launch("prep_image_kernel", MDATA_ERR_LAUNCH);
}

extern "C" int mdata_prep_label_u8(const uint8_t* src, int src_px, int src_ld, int in_h, int in_w, const int32_t* ytab,
                                   const int32_t* xtab, int rh, int rw, int y0, int x0, int ch, int cw, int flip,
                                   const uint8_t* lut1, const uint8_t* lut2, int32_t* hist, int64_t* out, int out_ld,
                                   void* stream) {
    MDATA_REQUIRE(src && out, "prep_label_u8: null src or out");
    MDATA_REQUIRE(src_px >= 1 && src_px <= 4, "prep_label_u8: pixel stride 1 .. 4 bytes, got %d", src_px);
    MDATA_REQUIRE(in_h > 0 && in_w > 0 && rh > 0 && rw > 0, "prep_label_u8: bad sizes in %d x %d -> %d x %d", in_h, in_w, rh, rw);
    MDATA_REQUIRE((long long)src_ld >= (long long)in_w * src_px, "prep_label_u8: src_ld %d bytes < in_w * src_px = %d", src_ld,
                  in_w * src_px);
    MDATA_REQUIRE((long long)in_h * src_ld < 0x7fffffffLL, "prep_label_u8: source of %d rows x %d bytes is too large", in_h, src_ld);
    MDATA_REQUIRE(ch > 0 && cw > 0 && y0 >= 0 && x0 >= 0 && (long long)y0 + ch <= rh && (long long)x0 + cw <= rw,
                  "prep_label_u8: crop %d x %d at (%d, %d) leaves the %d x %d image", ch, cw, y0, x0, rh, rw);
    MDATA_REQUIRE(ytab || rh == in_h, "prep_label_u8: no row table needs rh == in_h (%d vs %d)", rh, in_h);
    MDATA_REQUIRE(xtab || rw == in_w, "prep_label_u8: no column table needs rw == in_w (%d vs %d)", rw, in_w);
    MDATA_REQUIRE(aligned(ytab, 4) && aligned(xtab, 4) && aligned(hist, 4), "prep_label_u8: tables and hist must be 4-byte aligned");
    MDATA_REQUIRE(aligned(out, 8), "prep_label_u8: out must be 8-byte aligned");
    MDATA_REQUIRE(flip == 0 || flip == 1, "prep_label_u8: flip is 0 or 1, got %d", flip);
    MDATA_REQUIRE(out_ld >= cw, "prep_label_u8: out_ld %d < crop width %d", out_ld, cw);
    const unsigned gx = (unsigned)((cw + TX - 1) / TX), gy = (unsigned)((ch + LY - 1) / LY);
    MDATA_REQUIRE(gy <= 65535u, "prep_label_u8: crop of %d rows is too tall", ch);
    LabelGeom g{src_px, src_ld, in_h, in_w, y0, x0, ch, cw, flip, out_ld};
    prep_label_kernel<<<dim3(gx, gy), 256, 0, (hipStream_t)stream>>>(g, src, ytab, xtab, lut1, lut2, hist, out);
    return check_launch("prep_label_kernel", MDATA_ERR_LAUNCH);
}

extern "C" int mdata_png_unfilter(const uint8_t* in, size_t in_len, uint8_t* out, size_t out_len, int height,
                                  size_t row_bytes, int bpp) {
    int bad_row = -1;
    const int rc = png_unfilter_rows(in, in_len, out, out_len, height, row_bytes, bpp, &bad_row);
    if (rc == 1) {
        set_error("png_unfilter: inconsistent arguments (in %zu bytes, out %zu bytes, %d rows of %zu bytes, bpp %d)", in_len,
                  out_len, height, row_bytes, bpp);
        return MDATA_ERR_INVALID_ARG;
    }
    if (rc == 3) {
        set_error("png_unfilter: row %d has filter type %u (0 .. 4 exist)", bad_row,
                  (unsigned)in[(size_t)bad_row * (1 + row_bytes)]);
        return MDATA_ERR_FORMAT;
    }
    return MDATA_OK;
}
