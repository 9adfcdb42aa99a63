// Device arithmetic that several translation units, in more than one library, must form identically: each function has
// its one definition here (norm_bwd.hip, det.hip, spatial.hip, train.hip, vis.hip, headfuse.hip).  The deterministic mode's
// ordered sums (det.hip) are only bit-exact training because xh and dz there are the values madm_groupnorm_bwd_apply forms.
// Every function is forced inline: moving one here leaves each kernel's instructions as they were (tools/isa_diff.py).
#pragma once
#include <hip/hip_runtime.h>

// dy * act'(z); act: 0 none, 1 SiLU, 2 ReLU
__device__ __forceinline__ float act_grad_f(float z, float dy, int act) {
    if (act == 1) {
        const float sg = __builtin_amdgcn_rcpf(1.0f + __expf(-z));
        return dy * sg * (1.0f + z * (1.0f - sg));
    }
    if (act == 2) return z > 0.f ? dy : 0.f;
    return dy;
}

// per-channel {rstd_g, -mean_g * rstd_g} of the channels [c_off, c_off + C) of image b from the forward's channel
// sums; 8 lanes per group.  The caller synchronises.
__device__ __forceinline__ void gn_bwd_fold_stats(float* r, float* mr, int b, int HW, int C, int c_off, int Ctot, int G,
                                                  const double* __restrict__ sums1, int C1,
                                                  const double* __restrict__ sums2, float eps) {
    const int cpg = Ctot / G, C2 = Ctot - C1;
    const double inv_cnt = 1.0 / ((double)HW * (double)cpg);
    for (int g0 = 0; g0 < G; g0 += 32) {
        const int g = g0 + ((int)threadIdx.x >> 3), l = threadIdx.x & 7;
        double s = 0.0, q = 0.0;
        if (g < G) {
            for (int ch = g * cpg + l; ch < (g + 1) * cpg; ch += 8) {
                const double* src = (ch < C1) ? sums1 + ((size_t)b * C1 + ch) * 2 : sums2 + ((size_t)b * C2 + (ch - C1)) * 2;
                s += src[0];
                q += src[1];
            }
        }
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            s += __shfl_xor(s, o);
            q += __shfl_xor(q, o);
        }
        if (g < G) {
            const double mean = s * inv_cnt;
            double var = q * inv_cnt - mean * mean;
            if (var < 0.0) var = 0.0;
            const float rstd = __builtin_amdgcn_rsqf((float)var + eps);   // as the forward folds (norm.hip)
            for (int ch = g * cpg + l; ch < (g + 1) * cpg; ch += 8) {
                const int c = ch - c_off;
                if (c >= 0 && c < C) { r[c] = rstd; mr[c] = -(float)mean * rstd; }
            }
        }
    }
}

// PyTorch F.interpolate(mode='bilinear', align_corners=False) source index / weight
__device__ __forceinline__ void bilinear_coord(int o, int in_size, float scale, int& i0, int& i1, float& l1) {
    float src = ((float)o + 0.5f) * scale - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = (int)src;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = src - (float)i0;
}
