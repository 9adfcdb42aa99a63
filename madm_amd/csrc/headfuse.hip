// libmadm_headfuse.so (include/madm_headfuse.h): 2x bilinear upsample of the fused half-resolution map + concat with the
// projected s0 feature + the 1x1 classifier, in one pass -- the upsampled 256-channel map is never written.
//
// One workgroup (4 waves) owns 8 x 16 output pixels = MHF_TILE_H x MHF_TILE_W source pixels.  It copies the source tile
// with a one-pixel ring (indices clamped into the image, so every address below is valid) into LDS, 16-byte chunks, a
// pixel's row padded by one chunk.  Wave v owns output rows 2v, 2v + 1 of the tile: two MFMA pixel tiles of 16 pixels (one
// output row each).  Per K step a lane builds its B fragment -- pixel (lane & 15), chunk (lane >> 4) -- from the four
// source chunks in LDS: f32 blend with PyTorch's align_corners=False coordinates, ONE rounding to the compute dtype.  The A
// fragment is the packed classifier row (class = lane & 15 of the 16-class tile), read from global memory (a few KiB, shared
// by every workgroup: cache resident).  The C2 steps read the full-resolution operand straight from global memory.
// mma16 (common.hpp) leaves pixel = lane & 15, classes 4 (lane >> 4) .. + 3 in a lane: one 16-byte store per class tile.
#include "common.hpp"   // dtype traits, chunk conversion, mma16 (device helpers only: nothing here links to libmadm_hip.so)
#include "entry.hpp"
#include "madm_headfuse.h"
#include "shared_math.hpp"   // bilinear_coord

namespace {

#define MHF_REQUIRE(...) ENTRY_REQUIRE(MHF_ERR_INVALID_ARG, __VA_ARGS__)

constexpr int TH = MHF_TILE_H, TW = MHF_TILE_W, HALO_H = TH + 2, HALO_W = TW + 2;

struct Params {
    const void* hd;
    const void* proj;
    const void* w;
    const float* bias;
    float* out;
    int ldh, ldp, ldw, ldo;
    int B, h, w_lo, H, W, C1, C2, Kp;
};

template <typename T, int NT>
__global__ __launch_bounds__(256) void upsample_cat_classify_kernel(const Params p) {
    constexpr int EPC = TT<T>::EPC, KS = 4 * EPC;   // elements per chunk / per mma16 step
    extern __shared__ __attribute__((aligned(16))) uint4 halo[];   // [HALO_H * HALO_W][CPR + 1]
    const T* __restrict__ hd = static_cast<const T*>(p.hd);
    const T* __restrict__ proj = static_cast<const T*>(p.proj);
    const T* __restrict__ wgt = static_cast<const T*>(p.w);
    const int CPR = p.C1 / EPC, S = CPR + 1;
    const int b = blockIdx.z, ly0 = blockIdx.y * TH, lx0 = blockIdx.x * TW;

    for (int idx = threadIdx.x; idx < HALO_H * HALO_W * CPR; idx += 256) {
        const int q = idx % CPR, hp = idx / CPR;
        const int gy = min(max(ly0 - 1 + hp / HALO_W, 0), p.h - 1);
        const int gx = min(max(lx0 - 1 + hp % HALO_W, 0), p.w_lo - 1);
        halo[hp * S + q] = *reinterpret_cast<const uint4*>(hd + ((size_t)(b * p.h + gy) * p.w_lo + gx) * p.ldh + q * EPC);
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 15, g = lane >> 4;
    const int ox = 2 * lx0 + j, oxc = min(ox, p.W - 1);
    int x0, x1;
    float fx;
    bilinear_coord(oxc, p.w_lo, 0.5f, x0, x1, fx);   // the source is half the output
    x0 -= lx0 - 1;
    x1 -= lx0 - 1;

    int o00[2], o01[2], o10[2], o11[2];
    float w00[2], w01[2], w10[2], w11[2];
    size_t pix[2];
    bool live[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int oy = 2 * ly0 + 2 * wave + t, oyc = min(oy, p.H - 1);
        int y0, y1;
        float fy;
        bilinear_coord(oyc, p.h, 0.5f, y0, y1, fy);
        y0 -= ly0 - 1;
        y1 -= ly0 - 1;
        o00[t] = (y0 * HALO_W + x0) * S + g;
        o01[t] = (y0 * HALO_W + x1) * S + g;
        o10[t] = (y1 * HALO_W + x0) * S + g;
        o11[t] = (y1 * HALO_W + x1) * S + g;
        w00[t] = (1.f - fy) * (1.f - fx);
        w01[t] = (1.f - fy) * fx;
        w10[t] = fy * (1.f - fx);
        w11[t] = fy * fx;
        pix[t] = (size_t)(b * p.H + oyc) * p.W + oxc;
        live[t] = oy < p.H && ox < p.W;
    }

    const T* wrow[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wrow[nt] = wgt + (size_t)min(nt * 16 + j, p.Kp - 1) * p.ldw + g * EPC;

    f32x4 acc[2][NT];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[t][nt] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int steps1 = p.C1 / KS, steps2 = p.C2 / KS;
    for (int s = 0; s < steps1; ++s) {
        uint4 a[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) a[nt] = *reinterpret_cast<const uint4*>(wrow[nt] + s * KS);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float va[EPC], vb[EPC], vc[EPC], vd[EPC], o[EPC];
            chunk_to_f32<T>(halo[o00[t] + 4 * s], va);
            chunk_to_f32<T>(halo[o01[t] + 4 * s], vb);
            chunk_to_f32<T>(halo[o10[t] + 4 * s], vc);
            chunk_to_f32<T>(halo[o11[t] + 4 * s], vd);
#pragma unroll
            for (int e = 0; e < EPC; ++e) o[e] = w00[t] * va[e] + w01[t] * vb[e] + w10[t] * vc[e] + w11[t] * vd[e];
            const uint4 bf = f32_to_chunk<T>(o);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) mma16<T>(a[nt], bf, acc[t][nt]);
        }
    }
    for (int s = 0; s < steps2; ++s) {
        uint4 a[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) a[nt] = *reinterpret_cast<const uint4*>(wrow[nt] + p.C1 + s * KS);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const uint4 bf = *reinterpret_cast<const uint4*>(proj + pix[t] * p.ldp + s * KS + g * EPC);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) mma16<T>(a[nt], bf, acc[t][nt]);
        }
    }

#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int n = nt * 16 + 4 * g;
        if (n >= p.Kp) continue;
        const float4 bv = *reinterpret_cast<const float4*>(p.bias + n);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            if (!live[t]) continue;
            const f32x4 c = acc[t][nt];
            *reinterpret_cast<float4*>(p.out + pix[t] * p.ldo + n) = make_float4(c[0] + bv.x, c[1] + bv.y, c[2] + bv.z, c[3] + bv.w);
        }
    }
}

template <typename T>
int launch(const Params& p, hipStream_t s) {
    const dim3 grid((p.w_lo + TW - 1) / TW, (p.h + TH - 1) / TH, p.B);
    const size_t lds = (size_t)HALO_H * HALO_W * (p.C1 / TT<T>::EPC + 1) * sizeof(uint4);
    if (p.Kp <= 16)
        upsample_cat_classify_kernel<T, 1><<<grid, 256, lds, s>>>(p);
    else if (p.Kp <= 32)
        upsample_cat_classify_kernel<T, 2><<<grid, 256, lds, s>>>(p);
    else
        upsample_cat_classify_kernel<T, 4><<<grid, 256, lds, s>>>(p);
    return check_launch("upsample_cat_classify", MHF_ERR_LAUNCH);
}

}  // namespace

extern "C" {

int mhf_abi_version(void) { return 1; }
const char* mhf_last_error(void) { return g_err; }

int mhf_upsample_cat_classify(int dtype, const void* hd, int ldh, const void* proj, int ldp, const void* w, int ldw,
                              const float* bias, float* out, int ldo, int B, int h, int w_lo, int H, int W,
                              int C1, int C2, int Kp, void* stream) {
    MHF_REQUIRE(dtype == MHF_F32 || dtype == MHF_BF16 || dtype == MHF_F16, "upsample_cat_classify: unknown dtype %d", dtype);
    MHF_REQUIRE(hd && proj && w && bias && out, "upsample_cat_classify: null tensor pointer");
    MHF_REQUIRE(aligned(hd, 16) && aligned(proj, 16) && aligned(w, 16) && aligned(bias, 16) && aligned(out, 16),
                "upsample_cat_classify: hd / proj / w / bias / out must be 16-byte aligned");
    MHF_REQUIRE(B > 0 && h > 0 && w_lo > 0, "upsample_cat_classify: bad sizes B=%d h=%d w=%d", B, h, w_lo);
    MHF_REQUIRE(H == 2 * h && W == 2 * w_lo, "upsample_cat_classify: the output %d x %d is not twice the source %d x %d", H, W, h, w_lo);
    const int epc = dtype == MHF_F32 ? 4 : 8, es = dtype == MHF_F32 ? 4 : 2;
    MHF_REQUIRE(C1 > 0 && C1 % 32 == 0 && C1 <= MHF_MAX_ROW_BYTES / es,
                "upsample_cat_classify: unsupported width C1=%d (a multiple of 32, at most %d)", C1, MHF_MAX_ROW_BYTES / es);
    MHF_REQUIRE(C2 > 0 && C2 % 32 == 0, "upsample_cat_classify: unsupported width C2=%d (a multiple of 32)", C2);
    MHF_REQUIRE(Kp >= 4 && Kp % 4 == 0 && Kp <= MHF_MAX_CLASSES, "upsample_cat_classify: unsupported Kp=%d (a multiple of 4 in [4, %d])", Kp,
                MHF_MAX_CLASSES);
    MHF_REQUIRE(ldh >= C1 && ldh % epc == 0, "upsample_cat_classify: ldh=%d too small for %d channels or no multiple of %d", ldh, C1, epc);
    MHF_REQUIRE(ldp >= C2 && ldp % epc == 0, "upsample_cat_classify: ldp=%d too small for %d channels or no multiple of %d", ldp, C2, epc);
    MHF_REQUIRE(ldw >= C1 + C2 && ldw % epc == 0, "upsample_cat_classify: ldw=%d too small for %d columns or no multiple of %d", ldw,
                C1 + C2, epc);
    MHF_REQUIRE(ldo >= Kp && ldo % 4 == 0, "upsample_cat_classify: ldo=%d too small for %d classes or no multiple of 4", ldo, Kp);
    MHF_REQUIRE((long long)B * H * W < 0x7fffffffLL && B <= 65535 && (h + TH - 1) / TH <= 65535,
                "upsample_cat_classify: tensor too large (B * H * W < 2^31, B and h / %d at most 65535)", TH);
    const Params p{hd, proj, w, bias, out, ldh, ldp, ldw, ldo, B, h, w_lo, H, W, C1, C2, Kp};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == MHF_F32) return launch<float>(p, s);
    if (dtype == MHF_BF16) return launch<bf16_t>(p, s);
    return launch<f16_t>(p, s);
}

}  // extern "C"
