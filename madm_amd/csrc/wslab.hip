// libmadm_wslab.so (include/madm_wslab.h): the weight gradient of madm_conv2d_wgrad with its pixel slices kept and the order
// of every f32 addition fixed by the shapes.
//
// Stage 1 (wslab_kernel) is the block body of wgrad.hip's kernel -- a LOCAL COPY, the main loop unchanged line for line:
// moved into a shared header with the epilogue as a policy, the main library's three kernels were rescheduled (3 317 ->
// 3 378 instructions, 54 -> 58 SGPRs; tools/isa_diff.py), and that library's device code does not change for this mode
// (ln_rowstats_kernel of det.hip is the precedent).  A change to the loop in wgrad.hip is made here as
// well.  The epilogue is the store policy `Epi`: slice z = blockIdx.z stores its partial tile with plain stores to ws[z][n][k] and, the blocks of the
// first weight-column tile, its bias partial to wsb[z][n].  The bias partial is already reduced in a fixed order (a thread's
// staged rows in step order, the block's row slots in index order).  Stage 2 (wslab_fold_kernel): one thread per element of dw /
// dbias adds the slices in index order in f64 and updates the output once.  No atomics anywhere.
// Every (slice, tile) block of the grid runs at least one step (the slice count is recomputed from steps_per_slice), writes
// every element (n < N, k < K) of its tile -- and the fold reads exactly those.
#include "common.hpp"   // dtype traits, chunk conversion, mma16 (device helpers only: nothing here links to libmadm_hip.so)
#include "entry.hpp"
#include "madm_wslab.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

namespace {

struct WgradP {
    const char* in1; const char* in2; const char* dout; float* dw;
    int C1, C2, Ctot, ld1, ld2, ldd, B, IH, IW, OH, OW, KH, KW, stride, pad_t, pad_l, upsample;
    int N, K, M, steps_per_slice, lin;
    float* dbias;
    unsigned bytes1, bytes2, bytesd;
};

template <typename T, typename Epi>
__device__ __forceinline__ void conv2d_wgrad_body(const WgradP p, const Epi epi) {
    constexpr int EPC = TT<T>::EPC;
    constexpr int PX = 4 * EPC;                  // pixels per K step: one MFMA k-extent (bf16 32, f32 16)
    constexpr int CPR = 128 / EPC;               // 16-byte chunks per tile row
    constexpr int RPP = 256 / CPR;               // rows staged per pass of the block
    constexpr int LI = PX / RPP;                 // passes (2)
    constexpr int ROWB = 128 * (int)sizeof(T) + (sizeof(T) == 2 ? 32 : 16);   // padded: transposed reads conflict-free
    constexpr int TILEB = PX * ROWB;
    __shared__ __attribute__((aligned(16))) char smem[4 * TILEB];   // {dout, A} x 2 stages

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave & 1, wc = wave >> 1;
    const int fi = lane & 15, fg = lane >> 4;
    const int n0 = blockIdx.x * 128, kc0 = blockIdx.y * 128;
    const int cc = tid % CPR, r0 = tid / CPR;

    const int step0 = blockIdx.z * p.steps_per_slice;
    const int total_steps = (p.M + PX - 1) / PX;
    const int nsteps = min(p.steps_per_slice, total_steps - step0);
    if (nsteps <= 0) return;
    const int mend = (step0 + nsteps) * PX < p.M ? (step0 + nsteps) * PX : p.M;   // first pixel beyond this slice

    const __amdgpu_buffer_rsrc_t rsd = __builtin_amdgcn_make_buffer_rsrc((void*)p.dout, 0, p.bytesd, 0x00020000);
    // this thread's weight column: tap and channel are fixed, only the pixel moves
    const int kc = kc0 + cc * EPC;
    const bool kc_ok = kc < p.K;
    const int tap = kc_ok ? kc / p.Ctot : 0;
    const int c = kc - tap * p.Ctot;
    const int tr = tap / p.KW, ts = tap - tr * p.KW;
    const bool first = c < p.C1;
    const __amdgpu_buffer_rsrc_t rsa =
        first ? __builtin_amdgcn_make_buffer_rsrc((void*)p.in1, 0, p.bytes1, 0x00020000)
              : __builtin_amdgcn_make_buffer_rsrc((void*)p.in2, 0, p.bytes2, 0x00020000);
    const int lda = first ? p.ld1 : p.ld2;
    const int ca = first ? c : c - p.C1;
    const bool n_ok = n0 + cc * EPC < p.N;

    // output pixel of staged row i: m = (step0 + s) * PX + r0 + RPP * i, kept as (image, y, x) and advanced by PX
    int pm[LI], pb[LI], py[LI], px[LI];
#pragma unroll
    for (int i = 0; i < LI; ++i) {
        pm[i] = step0 * PX + r0 + RPP * i;
        const int q = pm[i] / p.OW;
        px[i] = pm[i] - q * p.OW;
        pb[i] = q / p.OH;
        py[i] = q - pb[i] * p.OH;
    }
    const int IHe = p.upsample ? 2 * p.IH : p.IH, IWe = p.upsample ? 2 * p.IW : p.IW;

    // Two register sets: the operands of step s + 2 are requested before step s is multiplied and written to LDS after
    // step s + 1 -- two MFMA phases of lead instead of none (one set: every step waited a full operand round trip, ~1 us
    // for 256 clocks of MFMA work: tools/exp/sweep_wgrad_splitm.py, one slice).  No condition around a request (steps past
    // the slice read out-of-range offsets = zeros, and are multiplied as zeros): the compiler keeps counted waits only in
    // straight-line code; three rotating sets under conditions made it drain every step.
    u32x4 rdA[LI], raA[LI], rdB[LI], raB[LI];
    auto load_step = [&](u32x4 (&rd)[LI], u32x4 (&ra)[LI]) {
#pragma unroll
        for (int i = 0; i < LI; ++i) {
            // branch-free per lane: an invalid row / column / tap position sets bit 31 of the offset (out of range for the
            // descriptor: zeros).  Written as "cond ? off : OOB" the compiler built two loads behind exec masks and had to
            // drain vmcnt between them (the address temporary shared the destination's registers).
            const bool m_ok = pm[i] < mend;   // (steps past the slice must not read the next slice's pixels)
            const unsigned badd = (unsigned)(!(m_ok && n_ok)) << 31;
            const unsigned offd = ((unsigned)(pm[i] * p.ldd + n0 + cc * EPC) * (unsigned)sizeof(T)) | badd;
            rd[i] = __builtin_amdgcn_raw_buffer_load_b128(rsd, offd, 0, 0);
            unsigned offa;
            bool a_ok = m_ok && kc_ok;
            if (p.lin) {   // uniform
                offa = (unsigned)(pm[i] * lda + ca) * (unsigned)sizeof(T);
            } else {
                int iy = py[i] * p.stride - p.pad_t + tr, ix = px[i] * p.stride - p.pad_l + ts;
                a_ok = a_ok && (unsigned)iy < (unsigned)IHe && (unsigned)ix < (unsigned)IWe;
                if (p.upsample) { iy >>= 1; ix >>= 1; }   // uniform
                offa = (unsigned)(((pb[i] * p.IH + iy) * p.IW + ix) * lda + ca) * (unsigned)sizeof(T);
            }
            ra[i] = __builtin_amdgcn_raw_buffer_load_b128(rsa, offa | ((unsigned)(!a_ok) << 31), 0, 0);
            pm[i] += PX;
            if (!p.lin) {   // (a linear layer is OW = 1: the walk below would take PX iterations per step for nothing)
                px[i] += PX;
                while (px[i] >= p.OW) {
                    px[i] -= p.OW;
                    if (++py[i] == p.OH) { py[i] = 0; ++pb[i]; }
                }
            }
        }
    };
    // bias gradient: the blocks of the first weight-column tile add up the dout chunks they stage (rows beyond M arrive
    // as zeros); reduced over the block's row slots at the end
    const bool do_bias = p.dbias != nullptr && blockIdx.y == 0;
    float bsum[EPC];
#pragma unroll
    for (int j = 0; j < EPC; ++j) bsum[j] = 0.f;
    auto store_step = [&](int stage, const u32x4 (&rd)[LI], const u32x4 (&ra)[LI]) {
        char* d = smem + stage * 2 * TILEB;
#pragma unroll
        for (int i = 0; i < LI; ++i) {
            const int off = (r0 + RPP * i) * ROWB + cc * 16;
            *reinterpret_cast<u32x4*>(d + off) = rd[i];
            *reinterpret_cast<u32x4*>(d + TILEB + off) = ra[i];
            if (do_bias) {
                float f[EPC];
                chunk_to_f32<T>(__builtin_bit_cast(uint4, rd[i]), f);
#pragma unroll
                for (int j = 0; j < EPC; ++j) bsum[j] += f[j];
            }
        }
    };

    f32x4 acc[4][4];   // [jn: 16 output channels][ic: 16 weight columns]
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[j][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    load_step(rdA, raA);   // step 0
    load_step(rdB, raB);   // step 1
    store_step(0, rdA, raA);
    __syncthreads();
    auto compute_step = [&](int stage) {
        const char* td = smem + stage * 2 * TILEB;
        const char* ta = td + TILEB;
        uint4 fd[4], fa[4];
        if constexpr (sizeof(T) == 2) {
            const int row = fg * 4 + (fi >> 2), colb = (fi & 3) * 8;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const char* q = td + row * ROWB + (wn * 64 + j * 16) * 2 + colb;
                const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)q);
                const s16x4 x1 =
                    __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(q + 16 * ROWB));
                const uint2 a0 = __builtin_bit_cast(uint2, x0), a1 = __builtin_bit_cast(uint2, x1);
                fd[j] = make_uint4(a0.x, a0.y, a1.x, a1.y);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const char* q = ta + row * ROWB + (wc * 64 + i * 16) * 2 + colb;
                const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)q);
                const s16x4 x1 =
                    __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(q + 16 * ROWB));
                const uint2 a0 = __builtin_bit_cast(uint2, x0), a1 = __builtin_bit_cast(uint2, x1);
                fa[i] = make_uint4(a0.x, a0.y, a1.x, a1.y);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const char* q = td + (fg * 4) * ROWB + (wn * 64 + j * 16 + fi) * 4;
                float4 v;
                v.x = *reinterpret_cast<const float*>(q);
                v.y = *reinterpret_cast<const float*>(q + ROWB);
                v.z = *reinterpret_cast<const float*>(q + 2 * ROWB);
                v.w = *reinterpret_cast<const float*>(q + 3 * ROWB);
                fd[j] = __builtin_bit_cast(uint4, v);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const char* q = ta + (fg * 4) * ROWB + (wc * 64 + i * 16 + fi) * 4;
                float4 v;
                v.x = *reinterpret_cast<const float*>(q);
                v.y = *reinterpret_cast<const float*>(q + ROWB);
                v.z = *reinterpret_cast<const float*>(q + 2 * ROWB);
                v.w = *reinterpret_cast<const float*>(q + 3 * ROWB);
                fa[i] = __builtin_bit_cast(uint4, v);
            }
        }
        // D[i][j] of mma16: i = row of the first operand (4 per lane), j = row of the second (lane & 15): the lane's
        // column index runs along the contiguous dim of dw
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) mma16<T>(fd[j], fa[i], acc[j][i]);
    };
    for (int s = 0; s < nsteps; s += 2) {
        load_step(rdA, raA);            // step s + 2
        compute_step(0);                // step s
        store_step(1, rdB, raB);        // step s + 1
        __syncthreads();
        load_step(rdB, raB);            // step s + 3
        compute_step(1);                // step s + 1 (zeros past the slice)
        store_step(0, rdA, raA);        // step s + 2
        __syncthreads();
    }

    if (do_bias) {   // (the loop's last barrier has passed: the staging LDS is free)
        float* red = reinterpret_cast<float*>(smem);
#pragma unroll
        for (int j = 0; j < EPC; ++j) red[r0 * 128 + cc * EPC + j] = bsum[j];
        __syncthreads();
        if (tid < 128 && n0 + tid < p.N) {
            float t = 0.f;
            for (int r = 0; r < RPP; ++r) t += red[r * 128 + tid];
            epi.bias(p, n0 + tid, t);
        }
    }

    // lane holds dw[n = nb + 4 fg + r][k = kb + fi]: one instruction covers 4 rows x 64 contiguous bytes
    epi.tile(p, acc, n0, kc0, wn, wc, fg, fi);
}


#define MWS_REQUIRE(...) ENTRY_REQUIRE(MWS_ERR_INVALID_ARG, __VA_ARGS__)

// ws / wsb: this launch's slabs [slices][N][K] and bias partials [slices][N]
struct SlabStore {
    float* ws;
    float* wsb;
    __device__ __forceinline__ void bias(const WgradP& p, int n, float t) const { wsb[(size_t)blockIdx.z * p.N + n] = t; }
    __device__ __forceinline__ void tile(const WgradP& p, const f32x4 (&acc)[4][4], int n0, int kc0, int wn, int wc, int fg,
                                         int fi) const {
        float* slab = ws + (size_t)blockIdx.z * p.N * p.K;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int n = n0 + wn * 64 + j * 16 + fg * 4;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = kc0 + wc * 64 + i * 16 + fi;
                if (k >= p.K) continue;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < p.N) slab[(size_t)(n + r) * p.K + k] = acc[j][i][r];
            }
        }
    }
};

template <typename T>
__global__ __launch_bounds__(256, 2) void wslab_kernel(const WgradP p, float* ws, float* wsb) {
    conv2d_wgrad_body<T>(p, SlabStore{ws, wsb});
}

// element idx < nk: dw[idx] and the slabs ws[z * nk + idx]; idx - nk < N (only with dbias): dbias and wsb[z * N + ..]
__global__ __launch_bounds__(256) void wslab_fold_kernel(const float* __restrict__ ws, const float* __restrict__ wsb, int slices,
                                                         size_t nk, int N, float* __restrict__ dw, float* __restrict__ dbias) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    const float* p;
    float* out;
    size_t step;
    if (idx < nk) {
        p = ws + idx; out = dw + idx; step = nk;
    } else if (dbias != nullptr && idx - nk < (size_t)N) {
        p = wsb + (idx - nk); out = dbias + (idx - nk); step = (size_t)N;
    } else {
        return;
    }
    double s = 0.0;
    int z = 0;
    for (; z + 8 <= slices; z += 8) {   // eight loads in flight, added in index order
        float t[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) t[u] = p[(size_t)(z + u) * step];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += (double)t[u];
    }
    for (; z < slices; ++z) s += (double)p[(size_t)z * step];
    *out = (float)((double)*out + s);
}

struct Geometry {
    int epc, px, total_steps, tilesN, tilesK, K, slices, steps_per_slice;
    long long M;
    size_t ws_bytes;
};

// The slice count of a launch: madm_conv2d_wgrad's rule (one round of resident blocks: MWS_TARGET_BLOCKS of them, at least 2
// steps per slice; for reductions of at most 512 steps the minimum of  rounds * steps per slice * 1 us + the cost of the partial tiles) with
// the partial tiles' cost restated for slabs: a slice's tile is one plain 64 KiB store and the fold's 64 KiB read of it
// (8 bytes of traffic per element at ~3 TB/s: ~2.7 ps -- an ESTIMATE from the traffic, not a fit; the main library's rule has
// 2.9 ps for its atomics and 4.2 for the sole owner's read-modify-write, both fitted); the fold's update of dw is there for every
// slice count, one included, and so is no term of the comparison.  Confirmed, not tuned, by tools/bench_backward.py --slabs
// --sweep: within 14 % of the best forced count on the fifteen shapes of the 512 x 512 step (worst: 512 -> 512 at 128 x 128, 255
// against 225 us at 8 slices; profiles/wslab_train_step.txt section 3).  Reads nothing but the shapes and the dtype.
int rule_slices(int total_steps, int tiles) {
    int sl = (MWS_TARGET_BLOCKS + tiles / 2) / tiles;
    const int cap = total_steps / 2;
    if (sl > cap) sl = cap;
    if (sl < 1) sl = 1;
    if (total_steps <= 512) {
        double best = 1e30;
        int bs = 1;
        for (int sm = 1; sm <= 32 && sm <= total_steps; ++sm) {
            const int per = (total_steps + sm - 1) / sm;
            const int blocks = tiles * ((total_steps + per - 1) / per);
            const int rounds = (blocks + 511) / 512;
            const double t = (double)rounds * per * 1.0 + (double)tiles * 16384.0 * sm * 2.7e-6;
            if (t < best) { best = t; bs = sm; }
        }
        sl = bs;
    }
    return sl;
}

// false: a size is out of range (no message: the queries return 0, the entry point has checked before)
bool geometry(const mws_conv2d_wgrad_args* a, Geometry* g) {
    if (!a || !(a->dtype == MWS_F32 || a->dtype == MWS_BF16 || a->dtype == MWS_F16)) return false;
    if (!(a->B > 0 && a->OH > 0 && a->OW > 0 && a->KH > 0 && a->KW > 0 && a->N > 0 && a->C1 > 0 && a->C2 >= 0 && a->slices >= 0))
        return false;
    g->epc = a->dtype == MWS_F32 ? 4 : 8;
    g->px = 4 * g->epc;
    const long long rows = (long long)a->B * a->OH, taps = (long long)a->KH * a->KW;      // (each product below stays in 64 bits)
    if (rows >= (1ll << 30) || taps >= (1ll << 30)) return false;
    g->M = rows * a->OW;
    const long long K = taps * ((long long)a->C1 + a->C2);
    if (g->M >= (1ll << 30) || K >= (1ll << 30)) return false;
    g->K = (int)K;
    g->total_steps = (int)((g->M + g->px - 1) / g->px);
    g->tilesN = (a->N + 127) / 128;
    g->tilesK = (g->K + 127) / 128;
    long long tiles = (long long)g->tilesN * g->tilesK;
    if (tiles > (1 << 30)) tiles = 1 << 30;
    int sl = a->slices > 0 ? a->slices : rule_slices(g->total_steps, (int)tiles);
    if (sl > g->total_steps) sl = g->total_steps;
    g->steps_per_slice = (int)((g->total_steps + sl - 1) / sl);
    g->slices = (g->total_steps + g->steps_per_slice - 1) / g->steps_per_slice;   // no empty slice
    const unsigned long long floats = (unsigned long long)g->slices * ((unsigned long long)a->N * g->K + a->N);
    if (floats >= (1ull << 40)) return false;
    g->ws_bytes = (size_t)floats * sizeof(float);
    return true;
}

}  // namespace

extern "C" {

int mws_abi_version(void) { return 1; }
const char* mws_last_error(void) { return g_err; }

int mws_conv2d_wgrad_slices(const mws_conv2d_wgrad_args* a) {
    Geometry g;
    return geometry(a, &g) ? g.slices : 0;
}

int mws_conv2d_wgrad_steps_per_slice(const mws_conv2d_wgrad_args* a) {
    Geometry g;
    return geometry(a, &g) ? g.steps_per_slice : 0;
}

size_t mws_conv2d_wgrad_workspace_bytes(const mws_conv2d_wgrad_args* a) {
    Geometry g;
    return geometry(a, &g) ? g.ws_bytes : 0;
}

int mws_conv2d_wgrad(const mws_conv2d_wgrad_args* a, void* stream) {
    MWS_REQUIRE(a && a->in1 && a->dout && a->dw && a->workspace, "conv2d_wgrad: null argument");
    MWS_REQUIRE(a->dtype == MWS_F32 || a->dtype == MWS_BF16 || a->dtype == MWS_F16, "conv2d_wgrad: unknown dtype %d", a->dtype);
    const int epc = a->dtype == MWS_F32 ? 4 : 8;
    const size_t esz = a->dtype == MWS_F32 ? 4 : 2;
    MWS_REQUIRE(a->C1 > 0 && a->C2 >= 0 && (a->C2 == 0 || a->in2), "conv2d_wgrad: bad channel split %d + %d", a->C1, a->C2);
    MWS_REQUIRE(a->C1 % epc == 0 && a->C2 % epc == 0, "conv2d_wgrad: C1 / C2 must be multiples of %d elements", epc);
    MWS_REQUIRE(a->N > 0 && a->N % 4 == 0, "conv2d_wgrad: N = %d must be a positive multiple of 4", a->N);
    MWS_REQUIRE(a->B > 0 && a->IH > 0 && a->IW > 0 && a->OH > 0 && a->OW > 0 && a->KH > 0 && a->KW > 0 && a->stride > 0,
                "conv2d_wgrad: bad geometry");
    MWS_REQUIRE(a->slices >= 0 && a->slices <= MWS_MAX_SLICES, "conv2d_wgrad: slices = %d outside [0, %d] (grid too large)", a->slices,
                MWS_MAX_SLICES);
    WgradP p;
    p.in1 = (const char*)a->in1; p.in2 = (const char*)a->in2; p.dout = (const char*)a->dout; p.dw = a->dw;
    p.C1 = a->C1; p.C2 = a->C2; p.Ctot = a->C1 + a->C2;
    p.ld1 = a->ld1 ? a->ld1 : a->C1;
    p.ld2 = a->ld2 ? a->ld2 : a->C2;
    p.ldd = a->ldd ? a->ldd : a->N;
    MWS_REQUIRE(p.ld1 % epc == 0 && p.ld2 % epc == 0 && p.ldd % 4 == 0, "conv2d_wgrad: row strides must keep 16-byte "
                "(dout: 8-byte) alignment");
    MWS_REQUIRE(aligned(a->in1, 16) && aligned(a->in2, 16), "conv2d_wgrad: in1 / in2 must be 16-byte aligned");
    MWS_REQUIRE(aligned(a->dout, 4 * esz), "conv2d_wgrad: dout must be aligned to %zu bytes", 4 * esz);
    MWS_REQUIRE(aligned(a->dw, 4) && aligned(a->dbias, 4), "conv2d_wgrad: dw / dbias must be 4-byte aligned");
    MWS_REQUIRE(aligned(a->workspace, 16), "conv2d_wgrad: workspace must be 16-byte aligned");
    p.B = a->B; p.IH = a->IH; p.IW = a->IW; p.OH = a->OH; p.OW = a->OW; p.KH = a->KH; p.KW = a->KW;
    p.stride = a->stride; p.pad_t = a->pad_t; p.pad_l = a->pad_l; p.upsample = a->upsample ? 1 : 0;
    p.N = a->N;
    p.dbias = a->dbias;
    Geometry g;
    MWS_REQUIRE(geometry(a, &g), "conv2d_wgrad: sizes out of range");
    p.K = g.K;
    const long long M = g.M;
    const long long in_rows = (long long)a->B * a->IH * a->IW;
    MWS_REQUIRE(M < (1ll << 30) && in_rows * p.ld1 * (long long)esz < (1ll << 31) &&
                    in_rows * (long long)p.ld2 * (long long)esz < (1ll << 31) && M * p.ldd * (long long)esz < (1ll << 31),
                "conv2d_wgrad: tensors must stay below 2 GiB");
    p.M = (int)M;
    p.bytes1 = (unsigned)(in_rows * p.ld1 * esz);
    p.bytes2 = a->C2 ? (unsigned)(in_rows * p.ld2 * esz) : 0u;
    p.bytesd = (unsigned)(M * p.ldd * esz);
    p.lin = (a->KH == 1 && a->KW == 1 && a->stride == 1 && a->pad_t == 0 && a->pad_l == 0 && !a->upsample && a->OH == a->IH &&
             a->OW == a->IW)
                ? 1 : 0;
    p.steps_per_slice = g.steps_per_slice;
    MWS_REQUIRE(g.slices <= MWS_MAX_SLICES && g.tilesK <= 65535, "conv2d_wgrad: grid too large");
    // the rule keeps a launch's slabs near MWS_TARGET_BLOCKS tiles of 64 KiB; a forced slice count may ask for more
    MWS_REQUIRE(g.ws_bytes < ((size_t)1 << 31), "conv2d_wgrad: the slabs need %zu bytes, at most 2 GiB are supported", g.ws_bytes);
    MWS_REQUIRE(a->workspace_bytes >= g.ws_bytes, "conv2d_wgrad: workspace of %zu bytes, %zu needed", a->workspace_bytes,
                g.ws_bytes);
    const size_t nk = (size_t)p.N * p.K;
    float* ws = static_cast<float*>(a->workspace);
    float* wsb = ws + (size_t)g.slices * nk;
    const dim3 grid((unsigned)g.tilesN, (unsigned)g.tilesK, (unsigned)g.slices);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (a->dtype == MWS_BF16) wslab_kernel<bf16_t><<<grid, 256, 0, s>>>(p, ws, wsb);
    else if (a->dtype == MWS_F16) wslab_kernel<f16_t><<<grid, 256, 0, s>>>(p, ws, wsb);
    else wslab_kernel<float><<<grid, 256, 0, s>>>(p, ws, wsb);
    if (int rc = check_launch("wslab_kernel", MWS_ERR_LAUNCH)) return rc;
    const size_t n = nk + (a->dbias ? (size_t)p.N : 0);
    wslab_fold_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(ws, wsb, g.slices, nk, p.N, a->dw, a->dbias);
    return check_launch("wslab_fold_kernel", MWS_ERR_LAUNCH);
}

}  // extern "C"
