// The periodic training picture (vis_period): one launch writes the whole RGB8 sheet from a table of up to 16 tile
// descriptors (include/madm_hip.h, madm_vis_compose).  The reference builds it on the host (.cpu() copies, F.interpolate
// + softmax + max per logits tile, PIL palettes, matplotlib: modeling/meta_arch/cmdise.py:238-305).  Byte traffic only:
// every thread produces 4 neighbouring pixels of one tile row (12 B out), the class planes of a logits tile are read
// coalesced along x, a low-resolution logits tile is sampled bilinearly per pixel and class (never materialised).  No LDS,
// no scratch: the table travels as kernel arguments and is read from there.
#include "common.hpp"
#include "shared_math.hpp"   // bilinear_coord

namespace {

struct VisTable {
    madm_vis_tile t[MADM_VIS_MAX_TILES];
};

constexpr int PX = 4;   // pixels per thread

__device__ __forceinline__ float clip01(float v) {
    v = (v != v) ? 0.f : v;
    return fminf(fmaxf(v, 0.f), 1.f);
}
// PX neighbouring f32 of one row: one 16-byte load where the row geometry allows it (W % 4 == 0, 16-byte aligned source)
__device__ __forceinline__ void load_px(const float* p, int npx, bool vec, float (&v)[PX]) {
    if (vec) {
        const float4 q = *reinterpret_cast<const float4*>(p);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int j = 0; j < PX; ++j) v[j] = (j < npx) ? p[j] : 0.f;
    }
}
__device__ __forceinline__ unsigned unit_to_byte(float v01) { return (unsigned)(int)floorf(fmaf(255.f, v01, 0.5f)); }

__global__ __launch_bounds__(256) void vis_compose_kernel(const VisTable tab, int n, int B, int H, int W, int cols_max,
                                                          int cols, int per_img,
                                                          const unsigned char* __restrict__ palette,
                                                          unsigned char* __restrict__ canvas) {
    const unsigned Wq = ((unsigned)W + PX - 1) / PX;
    const size_t per_cell = (size_t)H * Wq;
    const size_t total = (size_t)B * per_img * cols * per_cell;
    const size_t pitch = (size_t)cols * W * 3;
    for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
        // x fastest, then the cell column, then y, then the cell row: a wave walks along one canvas row
        const unsigned xq = (unsigned)(idx % Wq);
        size_t r = idx / Wq;
        const int cx = (int)(r % (unsigned)cols);
        r /= (unsigned)cols;
        const int y = (int)(r % (unsigned)H);
        const int cy = (int)(r / (unsigned)H);
        const int b = cy / per_img;
        const int ti = (cy - b * per_img) * cols_max + cx;
        const int x0 = (int)xq * PX;
        const int npx = min(PX, W - x0);

        unsigned char rgb[PX * 3];
#pragma unroll
        for (int j = 0; j < PX * 3; ++j) rgb[j] = 255;

        if (ti < n) {
            const int kind = tab.t[ti].kind;
            const void* src = tab.t[ti].src;
            const size_t HW = (size_t)H * W;
            const bool vec = (W & 3) == 0 && (((uintptr_t)src) & 15) == 0;
            if (kind == MADM_VIS_IMAGE) {
                const float sc = tab.t[ti].p0, sh = tab.t[ti].p1;
                const float* p = (const float*)src + (size_t)b * 3 * HW + (size_t)y * W + x0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    float v[PX];
                    load_px(p + c * HW, npx, vec, v);
#pragma unroll
                    for (int j = 0; j < PX; ++j)
                        rgb[j * 3 + c] = (unsigned char)unit_to_byte(clip01(__fadd_rn(__fmul_rn(v[j], sc), sh)));
                }
            } else if (kind == MADM_VIS_HEAT) {
                const float* p = (const float*)src + (size_t)b * HW + (size_t)y * W + x0;
                float v[PX];
                load_px(p, npx, vec, v);
#pragma unroll
                for (int j = 0; j < PX; ++j) {
                    const int t = (int)__fmul_rn(255.f, clip01(v[j]));
                    const float u = (float)t / 255.f;
                    const float u4 = 4.f * u;
                    rgb[j * 3 + 0] = (unsigned char)unit_to_byte(clip01(1.5f - fabsf(u4 - 3.f)));
                    rgb[j * 3 + 1] = (unsigned char)unit_to_byte(clip01(1.5f - fabsf(u4 - 2.f)));
                    rgb[j * 3 + 2] = (unsigned char)unit_to_byte(clip01(1.5f - fabsf(u4 - 1.f)));
                }
            } else {
                unsigned cls[PX];
                if (kind == MADM_VIS_LABEL) {
                    const int64_t* p = (const int64_t*)src + (size_t)b * HW + (size_t)y * W + x0;
#pragma unroll
                    for (int j = 0; j < PX; ++j) cls[j] = (j < npx) ? (unsigned)(p[j] & 255) : 0u;
                } else {   // MADM_VIS_LOGITS
                    const int K = tab.t[ti].C, h = tab.t[ti].h, w = tab.t[ti].w;
                    const size_t hw = (size_t)h * w;
                    const float* base = (const float*)src + (size_t)b * K * hw;
                    float best[PX];
#pragma unroll
                    for (int j = 0; j < PX; ++j) cls[j] = 0u;
                    if (h == H && w == W) {
                        const float* p = base + (size_t)y * W + x0;
                        for (int k = 0; k < K; ++k) {
                            float v[PX];
                            load_px(p + k * hw, npx, vec, v);
#pragma unroll
                            for (int j = 0; j < PX; ++j)
                                if (k == 0 || v[j] > best[j]) { best[j] = v[j]; cls[j] = (unsigned)k; }   // strict: first maximum
                        }
                    } else {
                        const float sy = (float)h / (float)H, sx = (float)w / (float)W;
                        int y0, y1;
                        float ly;
                        bilinear_coord(y, h, sy, y0, y1, ly);
                        int o00[PX], o01[PX], o10[PX], o11[PX];
                        float w00[PX], w01[PX], w10[PX], w11[PX];
#pragma unroll
                        for (int j = 0; j < PX; ++j) {
                            int xa, xb;
                            float lx;
                            bilinear_coord(min(x0 + j, W - 1), w, sx, xa, xb, lx);
                            o00[j] = y0 * w + xa; o01[j] = y0 * w + xb; o10[j] = y1 * w + xa; o11[j] = y1 * w + xb;
                            w00[j] = (1.f - ly) * (1.f - lx); w01[j] = (1.f - ly) * lx;
                            w10[j] = ly * (1.f - lx);         w11[j] = ly * lx;
                        }
                        for (int k = 0; k < K; ++k) {
                            const float* p = base + k * hw;
#pragma unroll
                            for (int j = 0; j < PX; ++j) {
                                const float v = w00[j] * p[o00[j]] + w01[j] * p[o01[j]] + w10[j] * p[o10[j]] + w11[j] * p[o11[j]];
                                if (k == 0 || v > best[j]) { best[j] = v; cls[j] = (unsigned)k; }
                            }
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < PX; ++j) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) rgb[j * 3 + c] = palette[cls[j] * 3 + c];
                }
            }
        }

        unsigned char* o = canvas + ((size_t)cy * H + y) * pitch + ((size_t)cx * W + x0) * 3;
        if (npx == PX && (((uintptr_t)o) & 3) == 0) {   // the pitch cols * W * 3 need not be a multiple of 4
            unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
            for (int q = 0; q < 3; ++q)
                o4[q] = (unsigned)rgb[q * 4] | ((unsigned)rgb[q * 4 + 1] << 8) | ((unsigned)rgb[q * 4 + 2] << 16) |
                        ((unsigned)rgb[q * 4 + 3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < PX; ++j) {
                if (j < npx) {
                    o[j * 3 + 0] = rgb[j * 3 + 0];
                    o[j * 3 + 1] = rgb[j * 3 + 1];
                    o[j * 3 + 2] = rgb[j * 3 + 2];
                }
            }
        }
    }
}

}  // namespace

extern "C" int madm_vis_compose(const madm_vis_tile* tiles, int n, int B, int H, int W, int cols_max,
                                const unsigned char* palette768, unsigned char* canvas, void* stream) {
    MADM_REQUIRE(tiles && palette768 && canvas, "vis_compose: null argument");
    MADM_REQUIRE(n >= 1 && n <= MADM_VIS_MAX_TILES, "vis_compose: 1 .. %d tiles, got %d", MADM_VIS_MAX_TILES, n);
    MADM_REQUIRE(B > 0 && H > 0 && W > 0 && cols_max > 0, "vis_compose: bad geometry B=%d H=%d W=%d cols_max=%d", B, H, W,
                 cols_max);
    VisTable tab = {};
    for (int i = 0; i < n; ++i) {
        const madm_vis_tile& t = tiles[i];
        MADM_REQUIRE(t.src, "vis_compose: tile %d has no source", i);
        MADM_REQUIRE(t.kind >= MADM_VIS_IMAGE && t.kind <= MADM_VIS_HEAT, "vis_compose: tile %d: unknown kind %d", i, t.kind);
        if (t.kind == MADM_VIS_LOGITS) {
            MADM_REQUIRE(t.C >= 1 && t.h > 0 && t.w > 0, "vis_compose: tile %d: bad logits shape [%d][%d][%d]", i, t.C, t.h, t.w);
            MADM_REQUIRE((size_t)t.C * t.h * t.w < 0x7fffffffull, "vis_compose: tile %d: logits too large for 32-bit plane offsets", i);
        } else {
            MADM_REQUIRE(t.h == H && t.w == W, "vis_compose: tile %d is %d x %d, the sheet's tiles are %d x %d (only logits are resized)",
                         i, t.h, t.w, H, W);
            MADM_REQUIRE(t.C == (t.kind == MADM_VIS_IMAGE ? 3 : 1), "vis_compose: tile %d: kind %d needs %d channel(s), got %d", i,
                         t.kind, t.kind == MADM_VIS_IMAGE ? 3 : 1, t.C);
        }
        tab.t[i] = t;
    }
    const int per_img = (n + cols_max - 1) / cols_max;
    const int cols = n < cols_max ? n : cols_max;
    const size_t total = (size_t)B * per_img * cols * H * (((size_t)W + PX - 1) / PX);
    size_t g = (total + 255) / 256;
    if (g > 8192) g = 8192;
    vis_compose_kernel<<<(unsigned)g, 256, 0, (hipStream_t)stream>>>(tab, n, B, H, W, cols_max, cols, per_img, palette768,
                                                                     canvas);
    return madm_check_launch("vis_compose_kernel");
}
