// C ABI of libmadm_wslab.so: the ordered-slab weight gradient of the deterministic training mode
// (madm_amd/ops.py: set_deterministic("slabs")).
//
// A library of its own next to libmadm_hip.so, loaded by the first weight gradient that takes the slab path.  Same style as
// madm_hip.h: raw pointers, explicit sizes and row strides in ELEMENTS, a hipStream_t passed as void*, an int status, no
// allocation and no ownership transfer.  On failure the message is in mws_last_error() (thread-local); argument errors are
// reported before anything touches the GPU.
//
//   dw[n][k] = (float)(dw[n][k] + sum_m dout[m][n] * A(m, k)),  k = (kh, kw, c), A = the gather of madm_conv2d_fwd
//
// madm_conv2d_wgrad splits the pixel range over grid slices that add their partial tiles with float atomics (order by
// scheduling), or runs ONE slice whose grid is the dw tiles alone.  mws_conv2d_wgrad keeps the slices and fixes the order.
// Two launches on the stream:
//   slabs   the main loop of madm_conv2d_wgrad's kernel; slice z stores its partial 128 x 128 tiles with plain stores to
//           workspace[z][n][k] (f32, N * K per slice) and the blocks of the first weight-column tile their bias partial to
//           workspace_bias[z][n] (behind the slabs: slices * N * K floats in).  No atomics.
//   fold    one thread per element of dw (and of dbias) adds the slices in index order in f64 and updates the output once.
// The workspace is a caller buffer of at least mws_conv2d_wgrad_workspace_bytes() bytes, 16-byte aligned; it is never read
// before it is written and nothing behind the queried size is touched.  The slice count and every other launch parameter
// depend on the shapes and the dtype only: not on the device, an occupancy query or the main library's tuning profile.
//
// dtype: 0 = f32, 1 = bf16, 2 = f16 (the values of madm_dtype).  Operand alignment and divisibility rules are those of
// madm_conv2d_wgrad_args, restated below.
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MWS_OK 0
#define MWS_ERR_INVALID_ARG 1
#define MWS_ERR_LAUNCH 2

#define MWS_F32 0
#define MWS_BF16 1
#define MWS_F16 2

#define MWS_MAX_SLICES 65535        /* grid.z */
#define MWS_TARGET_BLOCKS 640       /* the rule aims at one round of resident blocks: 2 per CU, a little oversubscribed */

typedef struct {
    int dtype;            /* of in1 / in2 / dout */
    const void* in1;      /* forward input [B, IH, IW, C1] (pixel stride ld1); 16-byte aligned */
    const void* in2;      /* second source or NULL; 16-byte aligned */
    int C1, C2;           /* multiples of 8 (16-bit) / 4 (f32) elements */
    int ld1, ld2;         /* 0 = dense; multiples of 16 bytes */
    const void* dout;     /* [M][ldd], M = B*OH*OW; aligned to 4 elements.  Read in 16-byte chunks: where N is not a multiple
                           * of the chunk the last chunk of a row covers up to 4 elements of what follows the window; they only
                           * feed rows n >= N of the product, which are never stored */
    int ldd;              /* 0 = dense (N); a multiple of 4 elements */
    float* dw;            /* f32 [N][KH*KW*(C1+C2)] dense, updated once per element; 4-byte aligned */
    int B, IH, IW, OH, OW, KH, KW, stride, pad_t, pad_l, upsample;
    int N;                /* multiple of 4 */
    float* dbias;         /* NULL or f32 [N] (4-byte aligned), updated once per element: sum over the M rows of dout */
    int slices;           /* pixel slices; 0 = the rule.  Clamped to the step count; no slice is empty */
    void* workspace;      /* at least workspace_bytes bytes, 16-byte aligned */
    size_t workspace_bytes;
} mws_conv2d_wgrad_args;

int mws_abi_version(void);          /* 1 */
const char* mws_last_error(void);

// The launch geometry of mws_conv2d_wgrad(a): read from dtype, the sizes and `slices` alone (no pointer is looked at).
// A reduction step is 32 pixels (16-bit) / 16 pixels (f32); slice z owns steps [z * steps_per_slice, (z + 1) *
// steps_per_slice) of ceil(M / pixels per step), the last slice what is left (at least one step).  0 on bad arguments.
int mws_conv2d_wgrad_slices(const mws_conv2d_wgrad_args* a);
int mws_conv2d_wgrad_steps_per_slice(const mws_conv2d_wgrad_args* a);
size_t mws_conv2d_wgrad_workspace_bytes(const mws_conv2d_wgrad_args* a);   /* slices * (N * K + N) * 4 */

int mws_conv2d_wgrad(const mws_conv2d_wgrad_args* a, void* stream);

#ifdef __cplusplus
}
#endif
