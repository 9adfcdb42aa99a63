// Shared by the halo-tile 3x3 convs -- conv3x3.hip (8 x 16 patches, register-staged weights), conv3x3_dma.hip (LDS-DMA weights)
// and conv3x3_h16.hip (16 x 16 patches): the block -> patch decode and the one launcher of all three; for the two 8 x 16 kernels
// also the patch geometry, the load of one halo chunk, its fused GroupNorm transform and the patch epilogue.
#pragma once
#include "igemm_common.hpp"

// Block index -> (output-channel tile, image, patch row, patch column) without run-time integer divisions: the three divisors
// are launch constants, so the host hands over their reciprocals m = ceil(2^32 / d) and the kernel takes q = umulhi(x, m),
// exact while x * d < 2^32 (checked by the launcher); d == 1 passes m = 0 and means q = x.  (Three 32-bit divisions are ~120
// VALU instructions in front of the first DMA of every block: 2.2 k clocks of set-up in the 8 x 16 kernel's stamps, round 4.)
struct PatchDecode {
    int patchesX, patchesPerImg;
    unsigned m_tilesN, m_ppi, m_px;
};
__host__ inline unsigned patch_magic(unsigned d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + d - 1) / d); }
__host__ inline bool patch_decode_fill(PatchDecode& pd, int patchesX, int patchesY, int tilesN, long long blocks) {
    pd.patchesX = patchesX; pd.patchesPerImg = patchesX * patchesY;
    pd.m_tilesN = patch_magic((unsigned)tilesN); pd.m_ppi = patch_magic((unsigned)pd.patchesPerImg);
    pd.m_px = patch_magic((unsigned)patchesX);
    const unsigned long long lim = 0x100000000ull;
    return (unsigned long long)blocks * (unsigned)tilesN < lim && (unsigned long long)blocks * (unsigned)pd.patchesPerImg < lim &&
           (unsigned long long)pd.patchesPerImg * (unsigned)patchesX < lim;
}
__device__ __forceinline__ int magic_div(int x, unsigned m) { return m ? (int)__umulhi((unsigned)x, m) : x; }
// Declares n0, b, py0, px0 of block `bid` (after xcd_block_order) of a grid of BN-channel tiles x PH x PW-pixel patches: first
// channel, image, patch origin (macro text: as an inline function it changed the 16 x 16 kernel's prologue)
#define HALO_PATCH_POS(BN, PH, PW, p, pd, bid)                                                  \
    const int tm = magic_div((bid), (pd).m_tilesN), tn = (bid) - tm * (p).tilesN;               \
    const int n0 = tn * (BN);                                                                   \
    const int b = magic_div(tm, (pd).m_ppi);                                                    \
    const int pr = tm - b * (pd).patchesPerImg;                                                 \
    const int pry = magic_div(pr, (pd).m_px);                                                   \
    const int py0 = pry * (PH), px0 = (pr - pry * (pd).patchesX) * (PW)

// The launch of a halo kernel: KERN = the instantiation (the once-per-device raise of its dynamic LDS is therefore per
// instantiation), on PH x PW-pixel patches and BN-channel tiles; `what` names the kernel family in error texts.
template <auto KERN, int BN, int PH, int PW>
int launch_halo_patches(const IgemmP& p0, size_t lds, hipStream_t s, const char* what, const char* kernel_name) {
    IgemmP p = p0;
    static std::atomic<uint64_t> attr_done{0};
    if (int e = madm_raise_dynamic_lds(reinterpret_cast<const void*>(KERN), lds, attr_done, what)) return e;
    const int patchesX = (p.OW + PW - 1) / PW, patchesY = (p.OH + PH - 1) / PH;
    p.tilesN = (p.N + BN - 1) / BN;
    dim3 grid((unsigned)(p.B * patchesX * patchesY * p.tilesN), 1, (unsigned)p.splitk);
    PatchDecode pd;
    if (!patch_decode_fill(pd, patchesX, patchesY, p.tilesN, (long long)grid.x)) {
        madm_set_error("%s: grid of %u blocks too large for the reciprocal patch decode", what, grid.x);
        return MADM_ERR_INVALID_ARG;
    }
    KERN<<<grid, 256, lds, s>>>(p, pd);
    return madm_check_launch(kernel_name);
}

namespace {

constexpr int TH = 8, TW = 16, HWD = TW + 2, HPIX = (TH + 2) * HWD;  // 180 halo pixels
#ifdef C3_STAMPS
__device__ unsigned long long g_c3_stamps[2048];
#endif

template <typename T, int EPC>
__device__ __forceinline__ u32x4 gn_act_chunk(u32x4 raw, const float* sc, const float* sh, int act) {
    float f[EPC];
    chunk_to_f32<T>(__builtin_bit_cast(uint4, raw), f);
#pragma unroll
    for (int j = 0; j < EPC; ++j) f[j] = f[j] * sc[j] + sh[j];
    act_inplace<EPC>(f, act);
    return __builtin_bit_cast(u32x4, f32_to_chunk<T>(f));
}

// {mean, rstd} of a channel's group folded into its staged gamma / beta: y = x * sc + sh with sc = rstd gamma, sh = beta - mean sc
__device__ __forceinline__ void gn_fold_affine(float2 st, float& sc, float& sh) {
    const float s = st.y * sc;
    sh = sh - st.x * s;
    sc = s;
}

// Requests halo chunk `ck` (HI 16-byte pieces per thread into hr[], zeros outside the map) and, FUSE, the raw gamma / beta of
// its channels into sc[] / sh[].  A macro over the kernel's locals, not a function: with the arrays passed by reference the
// compiler's alias analysis -- and with it the counted waits of conv3x3_dma.hip -- changed.
#define HALO_LOAD_CHUNK(ck)                                                                         \
    {                                                                                               \
        const int c0_ = (ck) * BKE;                                                                 \
        const bool first_ = c0_ < p.C1;                                                             \
        const __amdgpu_buffer_rsrc_t rs_ = first_ ? rs1 : rs2;                                      \
        const int ld_ = first_ ? p.ld1 : p.ld2;                                                     \
        const int cofs_ = (first_ ? c0_ : c0_ - p.C1) + cpos * EPC;                                 \
        _Pragma("unroll") for (int i = 0; i < HI; ++i) {                                            \
            const unsigned off_ = (unsigned)(pixoff[i] * ld_ + cofs_) * (unsigned)sizeof(T);        \
            hr[i] = __builtin_amdgcn_raw_buffer_load_b128(rs_, pixoff[i] >= 0 ? off_ : OOB, 0, 0);  \
        }                                                                                           \
        if (FUSE) {                                                                                 \
            const float* gs_ = p.gn_gamma + c0_ + cpos * EPC;   /* raw gamma / beta; the kernel's */ \
            const float* gh_ = p.gn_beta + c0_ + cpos * EPC;    /* STORE_HALO folds {mean, rstd} in */ \
            _Pragma("unroll") for (int j = 0; j < EPC; j += 4) {                                    \
                const float4 a_ = *reinterpret_cast<const float4*>(gs_ + j);                        \
                const float4 b_ = *reinterpret_cast<const float4*>(gh_ + j);                        \
                sc[j] = a_.x; sc[j + 1] = a_.y; sc[j + 2] = a_.z; sc[j + 3] = a_.w;                 \
                sh[j] = b_.x; sh[j + 1] = b_.y; sh[j + 2] = b_.z; sh[j + 3] = b_.w;                 \
            }                                                                                       \
        }                                                                                           \
    }

// ---- patch epilogue shared by the register-staged and the LDS-DMA halo kernels ----
// lane: pixel = patch row wm*4+i, column frow; channels n .. n+3.  ``red`` = >= 4 * BN floats of LDS nobody reads any more.
// PERM: the permuted channel mapping of igemm_tile_epilogue (igemm.hip) -- the LDS-DMA kernel fetches its weight rows in that order
// and the lane's 4 * NI channels are contiguous; the register-staged kernel keeps the plain mapping.
template <typename T, int BN, bool PERM = false>
__device__ __forceinline__ void halo_tile_epilogue(const IgemmP& p, f32x4 (&acc)[4][BN / 32], int b, int py0, int px0,
                                                   int n0, int z, float* red) {
    constexpr int MI = 4, NI = BN / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int frow = lane & 15, fg = lane >> 4;
    const bool want_stats = p.stats != nullptr && p.splitk == 1;
    constexpr int CS = PERM ? 4 : 16;
    const int lb = wn * (BN / 2) + fg * (PERM ? 4 * NI : 4);
    const int nb = n0 + lb;
    f32x4 cs[NI], cq[NI], add[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) { cs[j] = f32x4{0.f, 0.f, 0.f, 0.f}; cq[j] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    if (p.splitk == 1) epilogue_consts<NI, CS>(p, nb, b, add);   // a patch lies in one image
    int mrow[MI];
#pragma unroll
    for (int i = 0; i < MI; ++i) {
        const int oy = py0 + wm * 4 + i, ox = px0 + frow;
        mrow[i] = (oy < p.OH && ox < p.OW) ? (b * p.OH + oy) * p.OW + ox : -1;
    }
    if (p.splitk > 1) {
#pragma unroll
        for (int i = 0; i < MI; ++i) {
            if (mrow[i] < 0) continue;
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const f32x4 v = acc[i][j];
                if (nb + CS * j < p.N)
                    *reinterpret_cast<float4*>(p.ws + ((size_t)z * p.M + mrow[i]) * p.N + nb + CS * j) =
                        make_float4(v[0], v[1], v[2], v[3]);
            }
        }
    } else {
        epilogue_tile<T, MI, NI, CS>(p, mrow, nb, add, false, acc, PERM && EpiWide<T, NI>::ok(p));
        if (want_stats) {
#pragma unroll
            for (int i = 0; i < MI; ++i) {
                if (mrow[i] < 0) continue;
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    if (nb + CS * j < p.N) { cs[j] += acc[i][j]; cq[j] += acc[i][j] * acc[i][j]; }
            }
        }
    }
    if (want_stats) {
#pragma unroll
        for (int j = 0; j < NI; ++j) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                cs[j][r] = row16_sum(cs[j][r]);
                cq[j][r] = row16_sum(cq[j][r]);
            }
            if (frow == 0) {
                float* dst = red + ((wm * BN) + lb + CS * j) * 2;
#pragma unroll
                for (int r = 0; r < 4; ++r) { dst[2 * r] = cs[j][r]; dst[2 * r + 1] = cq[j][r]; }
            }
        }
    }
    if (want_stats) {
        __syncthreads();
        for (int c = tid; c < 2 * BN; c += 256) {
            const int n = n0 + (c >> 1);
            if (n < p.N)
                atomicAdd(p.stats + ((size_t)b * p.N + n0) * 2 + c, (double)red[c] + (double)red[2 * BN + c]);
        }
    }
}

}  // namespace
