// The evaluator's per-image export (evaluation/d2_evaluator.py:156-183 save_vis_results, eval_only): one launch writes the
// pixel data of all four files -- image, pred (16-bit), pred_color, gt_color -- already in PNG scanline form (filter byte 0,
// then the row's samples) into one contiguous byte buffer (include/madm_hip.h, madm_eval_export_pack).  The host only
// deflates slices of it.  Byte traffic only.  Rows are 1 + 3W / 1 + 2W bytes long, so no row and no plane starts aligned:
// the kernel is organised by OUTPUT word instead -- every thread owns one 4-byte-aligned word of the buffer, works out
// which (plane, row, column) each of its four bytes is and stores the word once; the up to three bytes in front of the
// first aligned word and behind the last one are byte stores of one extra thread.  No LDS, no scratch.
#include "common.hpp"

namespace {

struct PackGeom {
    unsigned H, W, HW;
    unsigned pitch3, pitch2;   // bytes per row of an RGB8 plane / of the 16-bit plane
    unsigned end0, end1, end2; // first byte offset behind the image / pred / pred_color plane
    unsigned total;
    int num_classes, ignore_label, image_u8;
};

// np.uint8(x) for x in [0, 255]: truncation toward zero; outside that range (undefined in numpy) the value saturates
__device__ __forceinline__ unsigned trunc_to_byte(float v) {
    v = (v != v) ? 0.f : v;
    return (unsigned)(int)fminf(fmaxf(v, 0.f), 255.f);
}

// the byte at offset ``off`` of the pack buffer; (last_px, last_cls) cache the class id of the pixel read last: the
// three colour bytes / two id bytes of one pixel are neighbours
__device__ __forceinline__ unsigned pack_byte(const PackGeom& g, unsigned off, const int64_t* __restrict__ pred,
                                              const int64_t* __restrict__ gt, const void* __restrict__ image,
                                              const unsigned char* __restrict__ palette, unsigned& last_px,
                                              unsigned& last_cls) {
    int plane;
    unsigned o, pitch;
    if (off < g.end0)      { plane = 0; o = off;          pitch = g.pitch3; }
    else if (off < g.end1) { plane = 1; o = off - g.end0; pitch = g.pitch2; }
    else if (off < g.end2) { plane = 2; o = off - g.end1; pitch = g.pitch3; }
    else                   { plane = 3; o = off - g.end2; pitch = g.pitch3; }
    const unsigned row = o / pitch, col = o - row * pitch;
    if (col == 0) return 0u;                                   // the row's filter byte: 0 = None
    const unsigned c = col - 1;
    if (plane == 0) {
        const unsigned x = c / 3u, ch = c - 3u * x;
        const size_t i = (size_t)ch * g.HW + (size_t)row * g.W + x;
        return g.image_u8 ? (unsigned)((const unsigned char*)image)[i] : trunc_to_byte(((const float*)image)[i]);
    }
    const unsigned x = plane == 1 ? (c >> 1) : c / 3u;
    const unsigned px = row * g.W + x;
    const unsigned key = px | (plane == 3 ? 0x80000000u : 0u);   // H * W < 2^31 is checked on the host
    if (key != last_px) {
        int64_t v;
        if (plane == 3) {
            v = gt[px];
            if (v == (int64_t)g.ignore_label) v = g.num_classes;   // d2_evaluator.py:122
        } else {
            v = pred[px];
        }
        last_px = key;
        last_cls = (unsigned)v;
    }
    if (plane == 1) return (c & 1u) ? (last_cls & 255u) : ((last_cls >> 8) & 255u);   // big-endian 16-bit sample
    return (unsigned)palette[(last_cls & 255u) * 3u + (c - 3u * x)];                  // .astype(np.uint8) -> 'P' -> RGB
}

__global__ __launch_bounds__(256) void eval_export_pack_kernel(const PackGeom g, const int64_t* __restrict__ pred,
                                                               const int64_t* __restrict__ gt,
                                                               const void* __restrict__ image,
                                                               const unsigned char* __restrict__ palette,
                                                               unsigned char* __restrict__ out, unsigned head,
                                                               unsigned nwords) {
    unsigned last_px = 0xffffffffu, last_cls = 0u;
    for (unsigned idx = blockIdx.x * 256u + threadIdx.x; idx <= nwords; idx += gridDim.x * 256u) {
        if (idx < nwords) {
            const unsigned off = head + 4u * idx;
            unsigned w = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= pack_byte(g, off + j, pred, gt, image, palette, last_px, last_cls) << (8 * j);
            *reinterpret_cast<unsigned*>(out + off) = w;
        } else {
            // the unaligned ends: bytes [0, head) and [head + 4 * nwords, total), at most three each
            for (unsigned off = 0; off < head; ++off)
                out[off] = (unsigned char)pack_byte(g, off, pred, gt, image, palette, last_px, last_cls);
            for (unsigned off = head + 4u * nwords; off < g.total; ++off)
                out[off] = (unsigned char)pack_byte(g, off, pred, gt, image, palette, last_px, last_cls);
        }
    }
}

}  // namespace

extern "C" int madm_eval_export_pack(const void* pred, const void* gt, const void* image, int image_kind,
                                     const unsigned char* palette768, int num_classes, int ignore_label, int H, int W,
                                     unsigned char* out, void* stream) {
    MADM_REQUIRE(pred && gt && image && palette768 && out, "eval_export_pack: null argument");
    MADM_REQUIRE(H > 0 && W > 0, "eval_export_pack: bad geometry H=%d W=%d", H, W);
    MADM_REQUIRE(image_kind == MADM_EXPORT_IMAGE_F32 || image_kind == MADM_EXPORT_IMAGE_U8,
                 "eval_export_pack: unknown image kind %d (0 = f32, 1 = u8)", image_kind);
    MADM_REQUIRE(num_classes >= 1 && num_classes <= 255, "eval_export_pack: 1 .. 255 classes, got %d", num_classes);
    const size_t total = (size_t)H * (4 + 11 * (size_t)W);
    MADM_REQUIRE(total < 0x7fffffffull, "eval_export_pack: %d x %d needs %zu bytes, more than 32-bit offsets hold", H, W, total);
    PackGeom g;
    g.H = (unsigned)H;
    g.W = (unsigned)W;
    g.HW = g.H * g.W;
    g.pitch3 = 1u + 3u * g.W;
    g.pitch2 = 1u + 2u * g.W;
    g.end0 = g.H * g.pitch3;
    g.end1 = g.end0 + g.H * g.pitch2;
    g.end2 = g.end1 + g.H * g.pitch3;
    g.total = (unsigned)total;
    g.num_classes = num_classes;
    g.ignore_label = ignore_label;
    g.image_u8 = image_kind == MADM_EXPORT_IMAGE_U8;
    unsigned head = (unsigned)((4u - (unsigned)((uintptr_t)out & 3u)) & 3u);
    if (head > g.total) head = g.total;
    const unsigned nwords = (g.total - head) / 4u;
    size_t blocks = ((size_t)nwords + 1 + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    eval_export_pack_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(
        g, (const int64_t*)pred, (const int64_t*)gt, image, palette768, out, head, nwords);
    return madm_check_launch("eval_export_pack_kernel");
}
