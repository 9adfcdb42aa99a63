// C ABI of libmadm_det.so: the fixed-order f32 reductions of the deterministic training mode (madm_amd/ops.py:
// set_deterministic).
//
// A library of its own next to libmadm_hip.so.  Every entry point replaces one reduction whose f32 additions the main
// library orders by scheduling (float atomics in LDS or in memory) with the same reduction in ONE order that is a function
// of the shapes alone.  Same style as madm_hip.h: raw pointers, explicit sizes and row strides in ELEMENTS, a hipStream_t
// passed as void*, an int status, no allocation and no ownership transfer.  On failure the message is in
// mdet_last_error() (thread-local); argument errors are reported before anything touches the GPU.
//
// All launching entry points are two stages on the stream:
//   partials  a workgroup owns a contiguous row slice of one image; a thread owns one 16-byte column chunk and one row
//             lane, walks its rows in increasing order adding in f32; the row lanes of a chunk are combined in lane order
//             by one thread (plain LDS stores, a barrier -- no atomics) and the block's partial is stored to
//             workspace[image][slice][column] with a plain store.
//   fold      one thread per (image, column) adds the slices in index order in f64 and performs the one update of the output.
// The workspace is a caller buffer of at least mdet_*_workspace_bytes(...) bytes, 16-byte aligned; it is never read
// before it is written.  Slice counts (mdet_*_slices) and every other launch parameter depend on the shapes only: not on
// the device, an occupancy query or the main library's tuning profile.
//
// dtype: 0 = f32, 1 = bf16, 2 = f16 (the values of madm_dtype).  x / dy / every 16-bit-or-f32 tensor operand is addressed in
// 16-byte chunks: 16-byte aligned, C and every row stride a multiple of the chunk (4 elements f32, 8 otherwise).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MDET_OK 0
#define MDET_ERR_INVALID_ARG 1
#define MDET_ERR_LAUNCH 2

#define MDET_F32 0
#define MDET_BF16 1
#define MDET_F16 2

#define MDET_MIN_SLICE_ROWS 16      /* a slice is never shorter than this unless the image is */
#define MDET_MAX_SLICES 1024        /* per launch, over all images (256 for the 9-sum depthwise gradient) */

int mdet_abi_version(void);         /* 1 */
const char* mdet_last_error(void);

// Row slices per image of a reduction over `rows` rows per image and `B` images (what mdet_colsum,
// mdet_groupnorm_stats, mdet_groupnorm_bwd_sums use with rows = HW; mdet_layernorm_bwd_params with rows = M, B = 1), and
// of mdet_dwconv3x3_wgrad (one "image" of B * H * W pixel rows).  0 on bad arguments.
int mdet_slices(int B, int rows);
int mdet_dwconv3x3_wgrad_slices(int B, int H, int W);

size_t mdet_colsum_workspace_bytes(int B, int HW, int C);
size_t mdet_groupnorm_stats_workspace_bytes(int B, int HW, int C);
size_t mdet_groupnorm_bwd_sums_workspace_bytes(int B, int HW, int C);
size_t mdet_layernorm_bwd_params_workspace_bytes(int M, int C);
size_t mdet_dwconv3x3_wgrad_workspace_bytes(int B, int H, int W, int C);

// out[b][c] = (float)(out[b][c] + sum_r x[(b * HW + r) * ldx + c]); out f32 [B][C], 4-byte aligned.
int mdet_colsum(int dtype, const void* x, int ldx, int B, int HW, int C, float* out,
                void* workspace, size_t workspace_bytes, void* stream);

// chsums[b][c][0] += sum_r x, chsums[b][c][1] += sum_r x * x; x dense [B * HW][C]; chsums f64 [B][C][2], 8-byte aligned.
int mdet_groupnorm_stats(int dtype, const void* x, int B, int HW, int C, double* chsums,
                         void* workspace, size_t workspace_bytes, void* stream);

// The arguments and the bsums layout of madm_groupnorm_bwd_sums: per (image, channel) S1 = sum dz and S2 = sum dz * xh of
// the source window [c_off, c_off + C) of a Ctot-channel GroupNorm (statistics sums1 [B][C1][2], sums2 [B][Ctot - C1][2]
// or NULL when C1 == Ctot), dz = dy * act'(xh * gamma + beta), act 0 none / 1 SiLU / 2 ReLU; added to the f64
// bsums[b][c_off + c][2].  dy has row stride lddy and is read at column c_off.  C <= 3584.
int mdet_groupnorm_bwd_sums(int dtype, const void* x, const void* dy, int lddy, int B, int HW, int C, int c_off, int Ctot,
                            int G, const double* sums1, int C1, const double* sums2, const float* gamma,
                            const float* beta, float eps, int act, double* bsums,
                            void* workspace, size_t workspace_bytes, void* stream);

// dbeta[c] = (float)(dbeta[c] + sum_b bsums[b][c][0]), dgamma[c] = (float)(dgamma[c] + sum_b bsums[b][c][1]), b in index
// order, summed in f64, c in [0, Ctot).  One thread per channel; no workspace.
int mdet_groupnorm_bwd_params(const double* bsums, int B, int Ctot, float* dgamma, float* dbeta, void* stream);

// LayerNorm over the last dim of dense x / dy [M][C]: dgamma[c] = (float)(dgamma[c] + sum_m dy * xh), dbeta[c] likewise
// with sum_m dy; the row statistics are recomputed one wave per row as madm_layernorm_bwd does; dx is not written.
int mdet_layernorm_bwd_params(int dtype, const void* x, const void* dy, int M, int C, float eps, float* dgamma,
                              float* dbeta, void* workspace, size_t workspace_bytes, void* stream);

// dw[t][c] = (float)(dw[t][c] + sum_pixels dy[p][c] * x[p + offset_t][c]) of the depthwise dilated 3x3 conv, taps outside
// the image skipped; x dense [B * H * W][C], dy with row stride lddy, dw f32 [9][C].  Any dilation > 0.
int mdet_dwconv3x3_wgrad(int dtype, const void* x, const void* dy, int lddy, float* dw, int B, int H, int W, int C,
                         int dilation, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
