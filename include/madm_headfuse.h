// C ABI of libmadm_headfuse.so: the last step of DAFormerHead(final_fuse_vae_decoder_feat=True) in one pass
// (madm_amd/head.py).
//
// A library of its own next to libmadm_hip.so, loaded by the first flagged head that takes the fused route.  Same style
// as madm_hip.h: raw pointers, explicit sizes and row strides in ELEMENTS, a hipStream_t passed as void*, an int status, no
// allocation and no ownership transfer.  On failure the message is in mhf_last_error() (thread-local); argument errors are
// reported before anything touches the GPU.
//
//   out[(b, y, x)][n] = sum_c w[n][c] * up2x(hd)[(b, y, x)][c] + sum_c w[n][C1 + c] * proj[(b, y, x)][c] + bias[n]
//
// hd is the half-resolution map [B * h * w][ldh] (C1 channels), proj the full-resolution one [B * H * W][ldp] (C2
// channels), H = 2 h and W = 2 w, w the packed classifier [Kp][ldw] over the concatenation (C1 then C2 columns), bias f32
// [Kp], out f32 [B * H * W][ldo] (Kp columns written, nothing else).  up2x is F.interpolate(scale 2, bilinear,
// align_corners=False): per axis the weights 0.25 / 0.75 of the two nearest source rows, the source index clamped at the
// border; the four-tap value is formed in f32 and rounded ONCE to the compute dtype (not at all for f32), products
// accumulate in f32, the bias is added last.  A workgroup stages the (4 + 2) x (8 + 2) source pixels of its 8 x 16
// output pixels in LDS once: every source row serves its four output pixels from there.
//
// dtype: 0 = f32, 1 = bf16, 2 = f16 (the values of madm_dtype).  hd / proj / w are addressed in 16-byte chunks: 16-byte
// aligned, ldh / ldp / ldw multiples of the chunk (4 elements f32, 8 otherwise).  out and bias are 16-byte aligned, ldo a
// multiple of 4.  Supported widths: C1 and C2 positive multiples of 32, C1 rows of at most MHF_MAX_ROW_BYTES bytes (256
// channels f32, 512 channels 16-bit), Kp a multiple of 4 in [4, MHF_MAX_CLASSES].  B * H * W < 2^31.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MHF_OK 0
#define MHF_ERR_INVALID_ARG 1
#define MHF_ERR_LAUNCH 2

#define MHF_F32 0
#define MHF_BF16 1
#define MHF_F16 2

#define MHF_TILE_H 4                /* half-resolution rows of a workgroup tile (8 output rows) */
#define MHF_TILE_W 8                /* half-resolution columns of a workgroup tile (16 output columns) */
#define MHF_MAX_ROW_BYTES 1024      /* C1 * element size */
#define MHF_MAX_CLASSES 64          /* Kp */

int mhf_abi_version(void);          /* 1 */
const char* mhf_last_error(void);

int mhf_upsample_cat_classify(int dtype, const void* hd, int ldh, const void* proj, int ldp, const void* w, int ldw,
                              const float* bias, float* out, int ldo, int B, int h, int w_lo, int H, int W,
                              int C1, int C2, int Kp, void* stream);

#ifdef __cplusplus
}
#endif
