// libmadm_det.so (include/madm_det.h): the fixed-order reductions of the deterministic training mode.
//
// One two-stage skeleton, five element functors.  Stage 1 (partials_kernel): grid (slices, B); a workgroup owns the rows
// [r0, r1) of image b; threads = (16-byte column chunk, row lane) exactly as in the kernels these replace (norm.hip,
// norm_bwd.hip, wgrad.hip, train.hip), a thread adds its rows in increasing order in f32, U rows per trip with all their
// loads issued together.  Where those kernels let the row lanes meet through f32 LDS atomics, here every lane stores its
// sums to its own LDS slot, and after a barrier lane 0 of the chunk adds them in lane order and stores the block's
// partial to workspace[b][slice][accumulator][column].  Stage 2 (fold_kernel): one thread per (b, accumulator, column)
// adds the slices in index order in f64 and updates the output once.  No atomics anywhere; slices, lanes and trips depend
// on the shapes and the dtype only.  HBM-bound streaming kernels: nothing here is tuned beyond the load batching.
#include "common.hpp"   // dtype traits and chunk conversion (device helpers only: nothing here links to libmadm_hip.so)
#include "entry.hpp"
#include "madm_det.h"
#include "shared_math.hpp"   // act_grad_f, gn_bwd_fold_stats

namespace {

#define MDET_REQUIRE(...) ENTRY_REQUIRE(MDET_ERR_INVALID_ARG, __VA_ARGS__)

#define MDET_DISPATCH_DTYPE(dtype, ...)   \
    do {                                  \
        if ((dtype) == MDET_F32) {        \
            typedef float T;              \
            __VA_ARGS__;                  \
        } else if ((dtype) == MDET_BF16) {\
            typedef bf16_t T;             \
            __VA_ARGS__;                  \
        } else {                          \
            typedef f16_t T;              \
            __VA_ARGS__;                  \
        }                                 \
    } while (0)

inline bool dtype_ok(int dtype) { return dtype == MDET_F32 || dtype == MDET_BF16 || dtype == MDET_F16; }
inline int epc_of(int dtype) { return dtype == MDET_F32 ? 4 : 8; }

// ---- the shapes-only launch geometry ------------------------------------------------------------------------------------
struct Geom {
    int R, C, rows_per_slice, slices;   // R = rows per image
};

int slices_for(long long rows, int cap) {
    if (rows <= 0 || cap < 1) return 0;
    long long s = (rows + MDET_MIN_SLICE_ROWS - 1) / MDET_MIN_SLICE_ROWS;
    if (s > cap) s = cap;
    const long long per = (rows + s - 1) / s;
    return (int)((rows + per - 1) / per);
}
int image_cap(int B) { return B >= MDET_MAX_SLICES ? 1 : MDET_MAX_SLICES / B; }
constexpr int DW_MAX_SLICES = 256;   // nine sums per channel: a quarter of the slices keeps the workspace small

Geom geom_for(int R, int C, int slices) { return Geom{R, C, (R + slices - 1) / slices, slices}; }
size_t ws_floats(int B, int slices, int nacc, int C) { return (size_t)B * slices * nacc * C; }

// ---- stage 1 ----------------------------------------------------------------------------------------------------------
// F: NACC sums per channel, NLD 16-byte loads per row, U rows per trip, and
//   setup<T>(cst, b)            all 256 threads, before a barrier: per-channel constants of image b into LDS (may be empty)
//   column<T>(col, cst, q)      the thread's constants of chunk q into registers
//   load<T>(v, b, row, q)       the row's NLD loads
//   add<T>(acc, v, col, row)    acc[a][j] += ...
template <typename T, typename F>
__global__ __launch_bounds__(256) void partials_kernel(const F f, const Geom g, float* __restrict__ ws) {
    constexpr int EPC = TT<T>::EPC, NACC = F::NACC, NLD = F::NLD, U = F::U;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* comb = lds;              // [256][EPC]: one slot per thread
    float* cst = lds + 256 * EPC;   // the functor's
    const int b = blockIdx.y, slice = blockIdx.x;
    const int r0 = slice * g.rows_per_slice;
    const int r1 = min(r0 + g.rows_per_slice, g.R);
    f.template setup<T>(cst, b);
    __syncthreads();

    const int CPR = g.C / EPC;
    const int cols = CPR < 256 ? CPR : 256;
    const int rowlanes = 256 / cols;
    const int tx = threadIdx.x % cols, ty = threadIdx.x / cols;
    float* dst = ws + ((size_t)b * g.slices + slice) * NACC * g.C;
    for (int q0 = 0; q0 < CPR; q0 += cols) {   // block-uniform trip count: the barriers below are met by every thread
        const int q = q0 + tx;
        float acc[NACC][EPC];
#pragma unroll
        for (int a = 0; a < NACC; ++a)
#pragma unroll
            for (int j = 0; j < EPC; ++j) acc[a][j] = 0.f;
        if (ty < rowlanes && q < CPR) {
            typename F::Col col;
            f.template column<T>(col, cst, q);
            for (int row = r0 + ty; row < r1; row += U * rowlanes) {
                uint4 v[U][NLD];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int rr = row + u * rowlanes;
#pragma unroll
                    for (int i = 0; i < NLD; ++i) v[u][i] = make_uint4(0u, 0u, 0u, 0u);
                    if (rr < r1) f.template load<T>(v[u], b, rr, q);
                }
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int rr = row + u * rowlanes;
                    if (rr < r1) f.template add<T>(acc, v[u], col, rr);
                }
            }
        }
        // the row lanes of a chunk, in lane order (a lane without rows holds exact zeros)
#pragma unroll
        for (int a = 0; a < NACC; ++a) {
#pragma unroll
            for (int j = 0; j < EPC; ++j) comb[threadIdx.x * EPC + j] = acc[a][j];
            __syncthreads();
            if (ty == 0 && q < CPR) {
                float s[EPC];
#pragma unroll
                for (int j = 0; j < EPC; ++j) s[j] = comb[tx * EPC + j];
                for (int l = 1; l < rowlanes; ++l)
#pragma unroll
                    for (int j = 0; j < EPC; ++j) s[j] += comb[(l * cols + tx) * EPC + j];
#pragma unroll
                for (int j = 0; j < EPC; j += 4)
                    *reinterpret_cast<float4*>(dst + (size_t)a * g.C + q * EPC + j) = make_float4(s[j], s[j + 1], s[j + 2], s[j + 3]);
            }
            __syncthreads();
        }
    }
}

// ---- stage 2 ----------------------------------------------------------------------------------------------------------
// where sum (b, a, c) goes: f64  d[(b * d_ctot + d_coff + c) * 2 + a] += s, or f32  t = (float)((double)t + s) with
// t = f1[c] for a == 1 when f1 is given, else f0[b * f_bstride + a * f_astride + c]
struct FoldOut {
    double* d;
    int d_ctot, d_coff;
    float* f0;
    float* f1;
    long long f_bstride, f_astride;
};

__global__ __launch_bounds__(256) void fold_kernel(const float* __restrict__ ws, int B, int slices, int nacc, int C,
                                                   const FoldOut o) {
    const size_t n = (size_t)B * nacc * C;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int c = (int)(idx % (size_t)C);
    const int a = (int)((idx / (size_t)C) % (size_t)nacc);
    const int b = (int)(idx / ((size_t)C * nacc));
    const size_t step = (size_t)nacc * C;
    const float* p = ws + (size_t)b * slices * step + (size_t)a * C + c;
    double s = 0.0;
    int k = 0;
    for (; k + 8 <= slices; k += 8) {   // eight loads in flight, added in index order
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(size_t)(k + u) * step];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)t[u];
    }
    for (; k < slices; ++k) s += (double)p[(size_t)k * step];
    if (o.d) {
        double* t = o.d + ((size_t)b * o.d_ctot + o.d_coff + c) * 2 + a;
        *t = *t + s;
    } else {
        float* t = (a == 1 && o.f1) ? o.f1 + c : o.f0 + (size_t)b * o.f_bstride + (size_t)a * o.f_astride + c;
        *t = (float)((double)*t + s);
    }
}

struct NoCol {};

// ---- colsum -------------------------------------------------------------------------------------------------------------
struct ColsumF {
    static constexpr int NACC = 1, NLD = 1, U = 4;
    typedef NoCol Col;
    const void* x;
    int ldx, HW;
    template <typename T> __device__ void setup(float*, int) const {}
    template <typename T> __device__ void column(Col&, const float*, int) const {}
    template <typename T> __device__ void load(uint4* v, int b, int row, int q) const {
        v[0] = *reinterpret_cast<const uint4*>((const T*)x + ((size_t)b * HW + row) * ldx + q * TT<T>::EPC);
    }
    template <typename T> __device__ void add(float (*acc)[TT<T>::EPC], const uint4* v, const Col&, int) const {
        float f[TT<T>::EPC];
        chunk_to_f32<T>(v[0], f);
#pragma unroll
        for (int j = 0; j < TT<T>::EPC; ++j) acc[0][j] += f[j];
    }
};

// ---- GroupNorm forward statistics -----------------------------------------------------------------------------------------
struct GnStatsF {
    static constexpr int NACC = 2, NLD = 1, U = 4;
    typedef NoCol Col;
    const void* x;
    int HW, C;
    template <typename T> __device__ void setup(float*, int) const {}
    template <typename T> __device__ void column(Col&, const float*, int) const {}
    template <typename T> __device__ void load(uint4* v, int b, int row, int q) const {
        v[0] = *reinterpret_cast<const uint4*>((const T*)x + ((size_t)b * HW + row) * C + q * TT<T>::EPC);
    }
    template <typename T> __device__ void add(float (*acc)[TT<T>::EPC], const uint4* v, const Col&, int) const {
        float f[TT<T>::EPC];
        chunk_to_f32<T>(v[0], f);
#pragma unroll
        for (int j = 0; j < TT<T>::EPC; ++j) { acc[0][j] += f[j]; acc[1][j] += f[j] * f[j]; }
    }
};

// ---- GroupNorm backward sums ------------------------------------------------------------------------------------------------
// xh and dz are the values madm_groupnorm_bwd_apply forms from the same statistics: shared_math.hpp defines both once
struct GnCol {
    float cr[8], cm[8], cg[8], cb[8];
};

struct GnBwdSumsF {
    static constexpr int NACC = 2, NLD = 2, U = 4;
    typedef GnCol Col;
    const void* x;
    const void* dy;
    int lddy, HW, C, c_off, Ctot, G, C1, act;
    const double* sums1;
    const double* sums2;
    const float* gamma;
    const float* beta;
    float eps;
    template <typename T> __device__ void setup(float* cst, int b) const {   // r, mr, gamma, beta [C]
        for (int c = threadIdx.x; c < C; c += blockDim.x) {
            cst[2 * C + c] = gamma[c_off + c];
            cst[3 * C + c] = beta[c_off + c];
        }
        gn_bwd_fold_stats(cst, cst + C, b, HW, C, c_off, Ctot, G, sums1, C1, sums2, eps);
    }
    template <typename T> __device__ void column(Col& k, const float* cst, int q) const {
#pragma unroll
        for (int j = 0; j < TT<T>::EPC; ++j) {
            const int c = q * TT<T>::EPC + j;
            k.cr[j] = cst[c]; k.cm[j] = cst[C + c]; k.cg[j] = cst[2 * C + c]; k.cb[j] = cst[3 * C + c];
        }
    }
    template <typename T> __device__ void load(uint4* v, int b, int row, int q) const {
        v[0] = *reinterpret_cast<const uint4*>((const T*)x + ((size_t)b * HW + row) * C + q * TT<T>::EPC);
        v[1] = *reinterpret_cast<const uint4*>((const T*)dy + ((size_t)b * HW + row) * lddy + c_off + q * TT<T>::EPC);
    }
    template <typename T> __device__ void add(float (*acc)[TT<T>::EPC], const uint4* v, const Col& k, int) const {
        float xf[TT<T>::EPC], df[TT<T>::EPC];
        chunk_to_f32<T>(v[0], xf);
        chunk_to_f32<T>(v[1], df);
#pragma unroll
        for (int j = 0; j < TT<T>::EPC; ++j) {
            const float xh = xf[j] * k.cr[j] + k.cm[j];
            const float dz = act_grad_f(xh * k.cg[j] + k.cb[j], df[j], act);
            acc[0][j] += dz;
            acc[1][j] += dz * xh;
        }
    }
};

// one thread per channel: the images of bsums in index order
__global__ __launch_bounds__(256) void gn_bwd_params_kernel(const double* __restrict__ bsums, int B, int Ctot,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= Ctot) return;
    double s1 = 0.0, s2 = 0.0;
    for (int b = 0; b < B; ++b) {
        const double* src = bsums + ((size_t)b * Ctot + c) * 2;
        s1 += src[0];
        s2 += src[1];
    }
    dbeta[c] = (float)((double)dbeta[c] + s1);
    dgamma[c] = (float)((double)dgamma[c] + s2);
}

// ---- LayerNorm parameter gradients ----------------------------------------------------------------------------------------------
// Row statistics first, one wave per row with layernorm_bwd_kernel's arithmetic (norm_bwd.hip: lane sums over its chunks,
// xor shuffles, 1 / sqrtf) into st[row] = (mean, rstd); the skeleton then reads them per row.
// A local copy, not in shared_math.hpp: calling even the 1 / sqrtf through a shared helper reschedules this kernel.
template <typename T>
__global__ __launch_bounds__(256) void ln_rowstats_kernel(const T* __restrict__ x, int M, int C, float eps,
                                                          float2* __restrict__ st) {
    constexpr int EPC = TT<T>::EPC;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;   // whole waves
    const int CPR = C / EPC;
    const float invC = 1.0f / (float)C;
    const T* xr = x + (size_t)row * C;
    float s = 0.f;
    for (int q = lane; q < CPR; q += 64) {
        float f[EPC];
        chunk_to_f32<T>(*reinterpret_cast<const uint4*>(xr + q * EPC), f);
#pragma unroll
        for (int j = 0; j < EPC; ++j) s += f[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const float mean = s * invC;
    float v2 = 0.f;
    for (int q = lane; q < CPR; q += 64) {
        float f[EPC];
        chunk_to_f32<T>(*reinterpret_cast<const uint4*>(xr + q * EPC), f);
#pragma unroll
        for (int j = 0; j < EPC; ++j) { const float t = f[j] - mean; v2 += t * t; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v2 += __shfl_xor(v2, o);
    const float rstd = 1.0f / sqrtf(v2 * invC + eps);
    if (lane == 0) st[row] = make_float2(mean, rstd);
}

struct LnParamsF {
    static constexpr int NACC = 2, NLD = 3, U = 4;   // sums: dgamma (dy * xh), dbeta (dy)
    typedef NoCol Col;
    const void* x;
    const void* dy;
    const float2* st;
    int C;
    template <typename T> __device__ void setup(float*, int) const {}
    template <typename T> __device__ void column(Col&, const float*, int) const {}
    template <typename T> __device__ void load(uint4* v, int, int row, int q) const {
        v[0] = *reinterpret_cast<const uint4*>((const T*)x + (size_t)row * C + q * TT<T>::EPC);
        v[1] = *reinterpret_cast<const uint4*>((const T*)dy + (size_t)row * C + q * TT<T>::EPC);
        const float2 s = st[row];
        v[2].x = __float_as_uint(s.x);
        v[2].y = __float_as_uint(s.y);
    }
    template <typename T> __device__ void add(float (*acc)[TT<T>::EPC], const uint4* v, const Col&, int) const {
        float f[TT<T>::EPC], d[TT<T>::EPC];
        chunk_to_f32<T>(v[0], f);
        chunk_to_f32<T>(v[1], d);
        const float mean = __uint_as_float(v[2].x), rstd = __uint_as_float(v[2].y);
#pragma unroll
        for (int j = 0; j < TT<T>::EPC; ++j) {
            const float xh = (f[j] - mean) * rstd;
            acc[0][j] += d[j] * xh;
            acc[1][j] += d[j];
        }
    }
};

// ---- depthwise 3x3 weight gradient ------------------------------------------------------------------------------------------
// rows = the B * H * W pixels as one image; per pixel the dy chunk and the (up to) nine x chunks around it
struct DwWgradF {
    static constexpr int NACC = 9, NLD = 10, U = 1;
    typedef NoCol Col;
    const void* x;
    const void* dy;
    int lddy, H, W, C, dil;
    template <typename T> __device__ void setup(float*, int) const {}
    template <typename T> __device__ void column(Col&, const float*, int) const {}
    template <typename T> __device__ void load(uint4* v, int, int p, int q) const {
        const int ox = p % W, t = p / W;
        const int oy = t % H, bi = t / H;
        v[0] = *reinterpret_cast<const uint4*>((const T*)dy + (size_t)p * lddy + q * TT<T>::EPC);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int iy = oy + (r - 1) * dil;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                const int ix = ox + (s - 1) * dil;
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                    v[1 + r * 3 + s] = *reinterpret_cast<const uint4*>((const T*)x + (((size_t)bi * H + iy) * W + ix) * C +
                                                                       q * TT<T>::EPC);
            }
        }
    }
    template <typename T> __device__ void add(float (*acc)[TT<T>::EPC], const uint4* v, const Col&, int p) const {
        const int ox = p % W, oy = (p / W) % H;
        float d[TT<T>::EPC];
        chunk_to_f32<T>(v[0], d);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            if ((unsigned)(oy + (r - 1) * dil) >= (unsigned)H) continue;
#pragma unroll
            for (int s = 0; s < 3; ++s) {
                if ((unsigned)(ox + (s - 1) * dil) >= (unsigned)W) continue;
                float f[TT<T>::EPC];
                chunk_to_f32<T>(v[1 + r * 3 + s], f);
#pragma unroll
                for (int j = 0; j < TT<T>::EPC; ++j) acc[r * 3 + s][j] += d[j] * f[j];
            }
        }
    }
};

// ---- host side ------------------------------------------------------------------------------------------------------------------
// what every entry point checks of its chunked tensor shapes; no GPU call
int check_common(const char* what, int dtype, int B, long long rows, int C, const void* ws, size_t ws_bytes, size_t need) {
    MDET_REQUIRE(dtype_ok(dtype), "%s: unknown dtype %d", what, dtype);
    MDET_REQUIRE(B > 0 && B <= 65535 && rows > 0 && rows < (1ll << 30) && C > 0, "%s: bad sizes (B %d, rows %lld, C %d)", what,
                 B, rows, C);
    MDET_REQUIRE(C % epc_of(dtype) == 0, "%s: C = %d must be a multiple of %d elements (16-byte chunks)", what, C,
                 epc_of(dtype));
    MDET_REQUIRE(ws && aligned(ws, 16), "%s: the workspace is missing or not 16-byte aligned", what);
    MDET_REQUIRE(ws_bytes >= need, "%s: the workspace has %zu bytes, %zu are needed", what, ws_bytes, need);
    return MDET_OK;
}

template <typename F>
int run(const char* what, int dtype, const F& f, int B, int R, int C, int slices, size_t cst_floats, float* ws,
        const FoldOut& out, hipStream_t s) {
    const Geom g = geom_for(R, C, slices);
    const size_t lds = ((size_t)256 * epc_of(dtype) + cst_floats) * sizeof(float);
    MDET_REQUIRE(lds <= 64 * 1024, "%s: C = %d too large", what, C);
    const dim3 grid((unsigned)g.slices, (unsigned)B);
    MDET_DISPATCH_DTYPE(dtype, (partials_kernel<T, F><<<grid, 256, lds, s>>>(f, g, ws)));
    int rc = check_launch(what, MDET_ERR_LAUNCH);
    if (rc != MDET_OK) return rc;
    const size_t n = (size_t)B * F::NACC * C;
    fold_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(ws, B, g.slices, F::NACC, C, out);
    return check_launch(what, MDET_ERR_LAUNCH);
}

}  // namespace

extern "C" {

int mdet_abi_version(void) { return 1; }
const char* mdet_last_error(void) { return g_err; }

int mdet_slices(int B, int rows) { return B > 0 ? slices_for(rows, image_cap(B)) : 0; }
int mdet_dwconv3x3_wgrad_slices(int B, int H, int W) {
    return (B > 0 && H > 0 && W > 0) ? slices_for((long long)B * H * W, DW_MAX_SLICES) : 0;
}

size_t mdet_colsum_workspace_bytes(int B, int HW, int C) {
    return (B > 0 && C > 0) ? ws_floats(B, mdet_slices(B, HW), 1, C) * sizeof(float) : 0;
}
size_t mdet_groupnorm_stats_workspace_bytes(int B, int HW, int C) {
    return (B > 0 && C > 0) ? ws_floats(B, mdet_slices(B, HW), 2, C) * sizeof(float) : 0;
}
size_t mdet_groupnorm_bwd_sums_workspace_bytes(int B, int HW, int C) { return mdet_groupnorm_stats_workspace_bytes(B, HW, C); }
size_t mdet_layernorm_bwd_params_workspace_bytes(int M, int C) {   // partials, then the rows' (mean, rstd)
    return (M > 0 && C > 0) ? (ws_floats(1, mdet_slices(1, M), 2, C) + (size_t)2 * M) * sizeof(float) : 0;
}
size_t mdet_dwconv3x3_wgrad_workspace_bytes(int B, int H, int W, int C) {
    return C > 0 ? ws_floats(1, mdet_dwconv3x3_wgrad_slices(B, H, W), 9, C) * sizeof(float) : 0;
}

int mdet_colsum(int dtype, const void* x, int ldx, int B, int HW, int C, float* out, void* workspace,
                size_t workspace_bytes, void* stream) {
    MDET_REQUIRE(x && out, "colsum: null argument");
    const int rc = check_common("colsum", dtype, B, HW, C, workspace, workspace_bytes, mdet_colsum_workspace_bytes(B, HW, C));
    if (rc != MDET_OK) return rc;
    MDET_REQUIRE(aligned(x, 16) && aligned(out, 4), "colsum: x must be 16-byte aligned, out 4-byte aligned");
    MDET_REQUIRE(ldx % epc_of(dtype) == 0 && ldx >= C, "colsum: ldx = %d must be a multiple of %d and at least C", ldx,
                 epc_of(dtype));
    const ColsumF f{x, ldx, HW};
    const FoldOut o{nullptr, 0, 0, out, nullptr, C, 0};
    return run("colsum", dtype, f, B, HW, C, mdet_slices(B, HW), 0, (float*)workspace, o, (hipStream_t)stream);
}

int mdet_groupnorm_stats(int dtype, const void* x, int B, int HW, int C, double* chsums, void* workspace,
                         size_t workspace_bytes, void* stream) {
    MDET_REQUIRE(x && chsums, "groupnorm_stats: null argument");
    const int rc = check_common("groupnorm_stats", dtype, B, HW, C, workspace, workspace_bytes,
                                mdet_groupnorm_stats_workspace_bytes(B, HW, C));
    if (rc != MDET_OK) return rc;
    MDET_REQUIRE(aligned(x, 16) && aligned(chsums, 8), "groupnorm_stats: x must be 16-byte aligned, chsums 8-byte aligned");
    const GnStatsF f{x, HW, C};
    const FoldOut o{chsums, C, 0, nullptr, nullptr, 0, 0};
    return run("groupnorm_stats", dtype, f, B, HW, C, mdet_slices(B, HW), 0, (float*)workspace, o, (hipStream_t)stream);
}

int mdet_groupnorm_bwd_sums(int dtype, const void* x, const void* dy, int lddy, int B, int HW, int C, int c_off, int Ctot,
                            int G, const double* sums1, int C1, const double* sums2, const float* gamma,
                            const float* beta, float eps, int act, double* bsums, void* workspace, size_t workspace_bytes,
                            void* stream) {
    MDET_REQUIRE(x && dy && sums1 && gamma && beta && bsums, "groupnorm_bwd_sums: null argument");
    const int rc = check_common("groupnorm_bwd_sums", dtype, B, HW, C, workspace, workspace_bytes,
                                mdet_groupnorm_bwd_sums_workspace_bytes(B, HW, C));
    if (rc != MDET_OK) return rc;
    const int epc = epc_of(dtype);
    MDET_REQUIRE(aligned(x, 16) && aligned(dy, 16) && aligned(sums1, 8) && aligned(sums2, 8) && aligned(bsums, 8) &&
                     aligned(gamma, 4) && aligned(beta, 4),
                 "groupnorm_bwd_sums: x / dy must be 16-byte aligned, the f64 sums 8-byte, gamma / beta 4-byte");
    MDET_REQUIRE(lddy % epc == 0 && c_off % epc == 0, "groupnorm_bwd_sums: lddy / c_off must be multiples of %d elements", epc);
    MDET_REQUIRE(G > 0 && Ctot > 0 && Ctot % G == 0 && c_off >= 0 && c_off + C <= Ctot && lddy >= Ctot && C1 > 0 &&
                     C1 <= Ctot && (C1 == Ctot || sums2),
                 "groupnorm_bwd_sums: bad channel layout (C %d at %d of %d, lddy %d, G %d, C1 %d)", C, c_off, Ctot, lddy, G, C1);
    MDET_REQUIRE(act >= 0 && act <= 2, "groupnorm_bwd_sums: unknown act %d", act);
    const GnBwdSumsF f{x, dy, lddy, HW, C, c_off, Ctot, G, C1, act, sums1, sums2, gamma, beta, eps};
    const FoldOut o{bsums, Ctot, c_off, nullptr, nullptr, 0, 0};
    return run("groupnorm_bwd_sums", dtype, f, B, HW, C, mdet_slices(B, HW), (size_t)4 * C, (float*)workspace, o,
               (hipStream_t)stream);
}

int mdet_groupnorm_bwd_params(const double* bsums, int B, int Ctot, float* dgamma, float* dbeta, void* stream) {
    MDET_REQUIRE(bsums && dgamma && dbeta, "groupnorm_bwd_params: null argument");
    MDET_REQUIRE(B > 0 && Ctot > 0, "groupnorm_bwd_params: bad sizes (B %d, Ctot %d)", B, Ctot);
    MDET_REQUIRE(aligned(bsums, 8) && aligned(dgamma, 4) && aligned(dbeta, 4),
                 "groupnorm_bwd_params: bsums must be 8-byte aligned, dgamma / dbeta 4-byte aligned");
    gn_bwd_params_kernel<<<dim3((unsigned)((Ctot + 255) / 256)), 256, 0, (hipStream_t)stream>>>(bsums, B, Ctot, dgamma, dbeta);
    return check_launch("groupnorm_bwd_params", MDET_ERR_LAUNCH);
}

int mdet_layernorm_bwd_params(int dtype, const void* x, const void* dy, int M, int C, float eps, float* dgamma,
                              float* dbeta, void* workspace, size_t workspace_bytes, void* stream) {
    MDET_REQUIRE(x && dy && dgamma && dbeta, "layernorm_bwd_params: null argument");
    const int rc = check_common("layernorm_bwd_params", dtype, 1, M, C, workspace, workspace_bytes,
                                mdet_layernorm_bwd_params_workspace_bytes(M, C));
    if (rc != MDET_OK) return rc;
    MDET_REQUIRE(aligned(x, 16) && aligned(dy, 16) && aligned(dgamma, 4) && aligned(dbeta, 4),
                 "layernorm_bwd_params: x / dy must be 16-byte aligned, dgamma / dbeta 4-byte aligned");
    const int slices = mdet_slices(1, M);
    float2* st = reinterpret_cast<float2*>((float*)workspace + ws_floats(1, slices, 2, C));   // C % 4 == 0: 16-byte aligned
    hipStream_t s = (hipStream_t)stream;
    MDET_DISPATCH_DTYPE(dtype, (ln_rowstats_kernel<T><<<dim3((unsigned)((M + 3) / 4)), 256, 0, s>>>((const T*)x, M, C, eps, st)));
    const int rc2 = check_launch("layernorm_bwd_params", MDET_ERR_LAUNCH);
    if (rc2 != MDET_OK) return rc2;
    const LnParamsF f{x, dy, st, C};
    const FoldOut o{nullptr, 0, 0, dgamma, dbeta, 0, 0};
    return run("layernorm_bwd_params", dtype, f, 1, M, C, slices, 0, (float*)workspace, o, s);
}

int mdet_dwconv3x3_wgrad(int dtype, const void* x, const void* dy, int lddy, float* dw, int B, int H, int W, int C,
                         int dilation, void* workspace, size_t workspace_bytes, void* stream) {
    MDET_REQUIRE(x && dy && dw, "dwconv3x3_wgrad: null argument");
    MDET_REQUIRE(B > 0 && H > 0 && W > 0 && dilation > 0 && dilation < (1 << 20), "dwconv3x3_wgrad: bad sizes");
    const long long npix = (long long)B * H * W;
    const int rc = check_common("dwconv3x3_wgrad", dtype, 1, npix, C, workspace, workspace_bytes,
                                mdet_dwconv3x3_wgrad_workspace_bytes(B, H, W, C));
    if (rc != MDET_OK) return rc;
    MDET_REQUIRE(aligned(x, 16) && aligned(dy, 16) && aligned(dw, 4),
                 "dwconv3x3_wgrad: x / dy must be 16-byte aligned, dw 4-byte aligned");
    MDET_REQUIRE(lddy % epc_of(dtype) == 0 && lddy >= C, "dwconv3x3_wgrad: lddy = %d must be a multiple of %d and at least C",
                 lddy, epc_of(dtype));
    const DwWgradF f{x, dy, lddy, H, W, C, dilation};
    const FoldOut o{nullptr, 0, 0, dw, nullptr, 0, C};
    return run("dwconv3x3_wgrad", dtype, f, 1, (int)npix, C, mdet_dwconv3x3_wgrad_slices(B, H, W), 0, (float*)workspace, o,
               (hipStream_t)stream);
}

}  // extern "C"
