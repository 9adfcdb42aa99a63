// CLIP text encoder pieces the GEMM / LayerNorm kernels do not cover (HF CLIPTextModel, the SD-v1-4 text tower the
// reference runs once on '' at construction, modeling/meta_arch/ldm_diffusers.py:219-243): the token + position
// embedding gather, the causal self-attention over <= 128 tokens and quick_gelu.  All f32: the reference runs the
// encoder in fp32 outside autocast.
//
// Causal attention: one workgroup per (image, head, 16-query chunk), four waves.  The workgroup stages the K and V rows
// its queries can see (rows 0 .. min(chunk end, L) - 1, the causal prefix) into LDS with a 65-float row stride: lane j
// reading K[j][d] then hits bank (j + d) mod 64, conflict-free.  Each wave walks its query rows one at a time with one
// query element per lane (D = 64): the score of key j = lane (and j = lane + 64) is a 64-step FMA chain over d with
// q[d] broadcast by v_readlane; max / sum are wave reductions in f32; o[d] (lane d) = sum over j <= i of p_j V[j][d]
// with p_j broadcast the same way.  Keys j > i are never read: their weight is exactly zero.
#include "common.hpp"

namespace {

constexpr int TE_D = 64;            // head dim the attention kernel serves (CLIP ViT-L/14 text tower: 12 x 64)
constexpr int TE_LMAX = 128;        // longest sequence (two keys per lane)
constexpr int TE_CHUNK = 16;        // query rows per workgroup
constexpr int TE_WAVES = 4;
constexpr int TE_ROWF = TE_D + 1;   // LDS row stride in floats

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float lane_bcast(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}

__global__ __launch_bounds__(TE_WAVES * 64) void causal_attn_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                     const float* __restrict__ v, float* __restrict__ o,
                                                                     int ldq, int ldk, int ldv, int ldo, int H, int L,
                                                                     float scale) {
    extern __shared__ float te_smem[];
    const int h = blockIdx.x, b = blockIdx.y, r0 = blockIdx.z * TE_CHUNK;
    const int r1 = min(r0 + TE_CHUNK, L);       // query rows [r0, r1); keys [0, r1) are visible to them
    float* Ks = te_smem;
    float* Vs = te_smem + (size_t)r1 * TE_ROWF;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t row0 = (size_t)b * L;
    for (int e = tid; e < r1 * TE_D; e += TE_WAVES * 64) {
        const int r = e >> 6, d = e & 63;
        Ks[r * TE_ROWF + d] = k[(row0 + r) * ldk + (size_t)h * TE_D + d];
        Vs[r * TE_ROWF + d] = v[(row0 + r) * ldv + (size_t)h * TE_D + d];
    }
    __syncthreads();

    for (int i = r0 + wave; i < r1; i += TE_WAVES) {
        const float qd = q[(row0 + i) * ldq + (size_t)h * TE_D + lane];
        const int j0 = lane, j1 = lane + 64;
        const bool v0 = j0 <= i, v1 = j1 <= i;
        // lanes whose key is not visible (j > i; possibly not staged) read row 0 instead; their score is discarded below
        const float* k0 = Ks + (v0 ? j0 : 0) * TE_ROWF;
        const float* k1 = Ks + (v1 ? j1 : 0) * TE_ROWF;
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int d = 0; d < TE_D; ++d) {
            const float qv = lane_bcast(qd, d);
            s0 = fmaf(qv, k0[d], s0);
            s1 = fmaf(qv, k1[d], s1);
        }
        s0 = v0 ? s0 * scale : -INFINITY;
        s1 = v1 ? s1 * scale : -INFINITY;
        const float m = wave_max(fmaxf(s0, s1));      // key 0 is always visible: m is finite
        const float p0 = v0 ? expf(s0 - m) : 0.f;
        const float p1 = v1 ? expf(s1 - m) : 0.f;
        const float l = wave_sum(p0 + p1);
        float acc = 0.f;
        const int n0 = min(i + 1, 64);
        for (int j = 0; j < n0; ++j) acc = fmaf(lane_bcast(p0, j), Vs[j * TE_ROWF + lane], acc);
        for (int j = 64; j <= i; ++j) acc = fmaf(lane_bcast(p1, j - 64), Vs[j * TE_ROWF + lane], acc);
        o[(row0 + i) * ldo + (size_t)h * TE_D + lane] = acc / l;
    }
}

__global__ void token_embedding_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                       const float* __restrict__ pos, float* __restrict__ out, int L, int C, int vocab,
                                       size_t n) {
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (size_t)gridDim.x * blockDim.x) {
        const size_t row = e / C;
        const int c = (int)(e - row * C);
        const int i = (int)(row % L);
        const int64_t id = ids[row];
        // the host rejects ids outside the vocabulary before upload; a bad id reaching the device reads nothing and
        // leaves a NaN row
        out[e] = (id >= 0 && id < vocab) ? tok[(size_t)id * C + c] + pos[(size_t)i * C + c] : __builtin_nanf("");
    }
}

template <typename T>
__global__ void quick_gelu_kernel(const T* __restrict__ x, T* __restrict__ y, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float a = TT<T>::ld(x + i);
        TT<T>::st(y + i, a / (1.0f + expf(-1.702f * a)));
    }
}

unsigned te_grid(size_t n) {
    size_t g = (n + 255) / 256;
    return (unsigned)(g < 1 ? 1 : (g > 2048 ? 2048 : g));
}

}  // namespace

int madm_token_embedding(const int64_t* ids, int N, int L, const float* tok, int vocab, const float* pos, int n_pos,
                         int C, float* out, void* stream) {
    MADM_REQUIRE(ids && tok && pos && out, "token_embedding: null pointer");
    MADM_REQUIRE(N > 0 && L > 0 && C > 0 && vocab > 0, "token_embedding: bad sizes N=%d L=%d C=%d vocab=%d", N, L, C, vocab);
    MADM_REQUIRE(L <= n_pos, "token_embedding: %d tokens but only %d positions", L, n_pos);
    const size_t n = (size_t)N * L * C;
    token_embedding_kernel<<<te_grid(n), 256, 0, (hipStream_t)stream>>>(ids, tok, pos, out, L, C, vocab, n);
    return madm_check_launch("token_embedding_kernel");
}

int madm_causal_attention_fwd(const madm_attention_args* a, void* stream) {
    MADM_REQUIRE(a, "causal_attention: null args");
    MADM_REQUIRE(a->dtype == MADM_F32, "causal_attention: f32 only (dtype %d)", a->dtype);
    MADM_REQUIRE(a->q && a->k && a->v && a->o, "causal_attention: null pointer");
    MADM_REQUIRE(a->D == TE_D, "causal_attention: head dim %d (only %d is served)", a->D, TE_D);
    MADM_REQUIRE(a->Lq == a->Lk, "causal_attention: self-attention only (Lq %d != Lk %d)", a->Lq, a->Lk);
    MADM_REQUIRE(a->Lq >= 1 && a->Lq <= TE_LMAX, "causal_attention: sequence length %d outside 1..%d", a->Lq, TE_LMAX);
    MADM_REQUIRE(a->B >= 1 && a->H >= 1 && a->B <= 65535, "causal_attention: bad B %d / H %d", a->B, a->H);
    const int HD = a->H * a->D;
    MADM_REQUIRE(a->ldq >= HD && a->ldk >= HD && a->ldv >= HD && a->ldo >= HD,
                 "causal_attention: row strides (%d %d %d %d) below H*D = %d", a->ldq, a->ldk, a->ldv, a->ldo, HD);
    MADM_REQUIRE(a->scale > 0.f, "causal_attention: scale %g", (double)a->scale);
    const int L = a->Lq;
    const int chunks = (L + TE_CHUNK - 1) / TE_CHUNK;
    const size_t lds = (size_t)2 * L * TE_ROWF * sizeof(float);   // the last chunk stages all L rows
    static std::atomic<uint64_t> raised{0};
    if (int rc = madm_raise_dynamic_lds((const void*)causal_attn_kernel, lds, raised, "causal_attn_kernel")) return rc;
    dim3 grid(a->H, a->B, chunks);
    causal_attn_kernel<<<grid, TE_WAVES * 64, lds, (hipStream_t)stream>>>(
        (const float*)a->q, (const float*)a->k, (const float*)a->v, (float*)a->o, a->ldq, a->ldk, a->ldv, a->ldo, a->H, L,
        a->scale);
    return madm_check_launch("causal_attn_kernel");
}

int madm_quick_gelu(int dtype, const void* x, void* y, size_t n, void* stream) {
    MADM_REQUIRE(x && y && n > 0, "quick_gelu: bad args");
    hipStream_t s = (hipStream_t)stream;
    MADM_DISPATCH_DTYPE(dtype, (quick_gelu_kernel<T><<<te_grid(n), 256, 0, s>>>((const T*)x, (T*)y, n)));
    return madm_check_launch("quick_gelu_kernel");
}
