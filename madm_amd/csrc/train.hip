// Kernels the training step of the path adds around the conv / norm / attention gradient kernels (SURVEY.md 8 a9, a10,
// 8f rank 2; BASELINE config 4): the train-mode DAFormer head (Dropout2d, depthwise-conv weight gradient, bilinear
// resize adjoint), the CmdiseCriterion losses with their gradients (pixel-weighted cross entropy with ignore index,
// masked L1 / L2 on the latents) and the backward of the tanh-gated prompt / time conditioning.  In the reference all of
// these are torch autograd nodes behind ``losses.backward()`` (engine/train_loop.py:203-217).  HBM-bound streaming kernels.
#include "common.hpp"
#include "shared_math.hpp"   // bilinear_coord

namespace {

// y[b][p][c] = x[b][p][c] * s[b][c]: Dropout2d (s = keep-mask / (1 - p) per (image, channel)); its own backward on dy
template <typename T>
__global__ __launch_bounds__(256) void scale_channels_kernel(const T* __restrict__ x, int ldx, const float* __restrict__ s,
                                                             T* __restrict__ y, int ldy, int HW, int C, size_t total) {
    constexpr int EPC = TT<T>::EPC;
    const unsigned CPR = (unsigned)C / EPC;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned q = (unsigned)(idx % CPR);
        const size_t pix = idx / CPR;
        const size_t b = pix / (size_t)HW;
        float f[EPC];
        chunk_to_f32<T>(*reinterpret_cast<const uint4*>(x + pix * ldx + q * EPC), f);
        const float* sb = s + b * C + q * EPC;
#pragma unroll
        for (int j = 0; j < EPC; ++j) f[j] *= sb[j];
        *reinterpret_cast<uint4*>(y + pix * ldy + q * EPC) = f32_to_chunk<T>(f);
    }
}

// dx = dy where y > 0 (y = the ReLU's OUTPUT), else 0
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const T* __restrict__ y, const T* __restrict__ dy, T* __restrict__ dx,
                                                       size_t chunks) {
    constexpr int EPC = TT<T>::EPC;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < chunks; i += (size_t)gridDim.x * blockDim.x) {
        float a[EPC], d[EPC];
        chunk_to_f32<T>(reinterpret_cast<const uint4*>(y)[i], a);
        chunk_to_f32<T>(reinterpret_cast<const uint4*>(dy)[i], d);
#pragma unroll
        for (int j = 0; j < EPC; ++j) d[j] = a[j] > 0.f ? d[j] : 0.f;
        reinterpret_cast<uint4*>(dx)[i] = f32_to_chunk<T>(d);
    }
}

// weight gradient of the depthwise dilated 3x3 conv: dw[t][c] += sum_pixels dy[p][c] * x[p + off_t][c].
// grid = pixel slices; threads = (channel chunk, pixel lane); 9 x EPC register sums per thread -> LDS -> f32 atomics.
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_kernel(const T* __restrict__ x, const T* __restrict__ dy, int lddy,
                                                              float* __restrict__ dw, int B, int H, int W, int C, int dil,
                                                              int pix_per_block) {
    constexpr int EPC = TT<T>::EPC;
    extern __shared__ __attribute__((aligned(16))) float lds[];   // [9][C]
    for (int i = threadIdx.x; i < 9 * C; i += blockDim.x) lds[i] = 0.f;
    __syncthreads();
    const int CPR = C / EPC;
    const int cols = CPR < 256 ? CPR : 256;
    const int lanes = 256 / cols;
    const int tx = threadIdx.x % cols, ty = threadIdx.x / cols;
    const size_t npix = (size_t)B * H * W;
    const size_t p0 = (size_t)blockIdx.x * pix_per_block;
    size_t p1 = p0 + pix_per_block;
    if (p1 > npix) p1 = npix;
    if (ty < lanes) {
        for (int q = tx; q < CPR; q += cols) {
            float acc[9][EPC];
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int j = 0; j < EPC; ++j) acc[t][j] = 0.f;
            for (size_t p = p0 + ty; p < p1; p += lanes) {
                const int ox = (int)(p % (size_t)W);
                const size_t t_ = p / (size_t)W;
                const int oy = (int)(t_ % (size_t)H);
                const size_t b = t_ / (size_t)H;
                float d[EPC];
                chunk_to_f32<T>(*reinterpret_cast<const uint4*>(dy + p * lddy + q * EPC), d);
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const int iy = oy + (r - 1) * dil;
                    if ((unsigned)iy >= (unsigned)H) continue;
#pragma unroll
                    for (int s = 0; s < 3; ++s) {
                        const int ix = ox + (s - 1) * dil;
                        if ((unsigned)ix >= (unsigned)W) continue;
                        float f[EPC];
                        chunk_to_f32<T>(*reinterpret_cast<const uint4*>(x + ((b * H + iy) * W + ix) * C + q * EPC), f);
#pragma unroll
                        for (int j = 0; j < EPC; ++j) acc[r * 3 + s][j] += d[j] * f[j];
                    }
                }
            }
#pragma unroll
            for (int t = 0; t < 9; ++t)
#pragma unroll
                for (int j = 0; j < EPC; ++j) atomicAdd(&lds[t * C + q * EPC + j], acc[t][j]);
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 9 * C; i += blockDim.x) unsafeAtomicAdd(dw + i, lds[i]);
}

// The same gradient on the dilation's lattice (spatial.hip, dwconv3x3_lattice_kernel): a workgroup owns one residue
// class (ry, rx) of one image and one 128-byte channel slab and walks that class's tiles of at most 15 x 15 lattice
// pixels; per tile the x halo sits in LDS (1.27 global requests per element instead of 9), every thread multiplies its 8
// dy chunks with the 3 x 10 halo chunks around them into 9 x EPC register sums that live across the tiles; one LDS +
// global atomic round per workgroup (measurements at the launcher).
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3_wgrad_lattice_kernel(const T* __restrict__ x, const T* __restrict__ dy, int lddy,
                                                                      float* __restrict__ dw, int B, int H, int W, int C, int dil,
                                                                      int ny, int nx, int th, int tw) {
    constexpr int EPC = TT<T>::EPC;
    constexpr int CHS = 8 * EPC;
    __shared__ __attribute__((aligned(16))) uint4 halo[17 * 17 * 8];   // tiles of at most 15 x 15: 37 KB, four workgroups per CU
    __shared__ float red[9 * CHS];
    const int tid = threadIdx.x;
    unsigned t = blockIdx.x;
    const int slabs = C / CHS;
    const int slab = (int)(t % (unsigned)slabs); t /= (unsigned)slabs;
    const int rx = (int)(t % (unsigned)dil); t /= (unsigned)dil;
    const int ry = (int)(t % (unsigned)dil);
    const int b = (int)(t / (unsigned)dil);
    const int c0 = slab * CHS;
    const int hw_ = tw + 2, items = (th + 2) * hw_ * 8;
    const int q = tid & 7, g = tid >> 3;
    const int r = g >> 1, half = g & 1;
    for (int i = tid; i < 9 * CHS; i += 256) red[i] = 0.f;
    float acc[9][EPC];
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < EPC; ++j) acc[k][j] = 0.f;
    constexpr int MAXP = (17 * 17 * 8 + 255) / 256;
    for (int tile = 0; tile < ny * nx; ++tile) {
        const int ty = tile / nx, tx = tile - ty * nx;
        const int sy0 = ty * th, sx0 = tx * tw;
        uint4 hv[MAXP];
#pragma unroll
        for (int k = 0; k < MAXP; ++k) {
            const int i = tid + 256 * k;
            hv[k] = make_uint4(0u, 0u, 0u, 0u);
            if (i < items) {
                const int hp = i >> 3, qq = i & 7;
                const int hy = hp / hw_, hx = hp - hy * hw_;
                const int iy = ry + dil * (sy0 + hy - 1), ix = rx + dil * (sx0 + hx - 1);
                if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W)
                    hv[k] = *reinterpret_cast<const uint4*>(x + (((size_t)b * H + iy) * W + ix) * C + c0 + qq * EPC);
            }
        }
        // the thread's 8 dy chunks: row r of the tile, columns half * 8 .. + 7 (zeros outside the tile / the image)
        const int oy = ry + dil * (sy0 + r);
        const bool row_on = r < th && oy < H;
        uint4 dv[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const int sx = half * 8 + o;
            const int ox = rx + dil * (sx0 + sx);
            dv[o] = make_uint4(0u, 0u, 0u, 0u);
            if (row_on && sx < tw && ox < W)
                dv[o] = *reinterpret_cast<const uint4*>(dy + (((size_t)b * H + oy) * W + ox) * lddy + c0 + q * EPC);
        }
        __syncthreads();   // the previous tile's halo has been read by every wave
#pragma unroll
        for (int k = 0; k < MAXP; ++k) {
            const int i = tid + 256 * k;
            if (i < items) halo[i] = hv[k];
        }
        __syncthreads();
        if (row_on) {
#pragma unroll
            for (int rr = 0; rr < 3; ++rr) {
                const uint4* hrow = halo + ((r + rr) * hw_ + half * 8) * 8 + q;
#pragma unroll
                for (int c = 0; c < 10; ++c) {      // halo column half * 8 + c meets outputs c - s under tap (rr, s)
                    if (half * 8 + c < hw_) {       // (pixels outside the image hold zeros in the halo)
                        float f[EPC];
                        chunk_to_f32<T>(hrow[c * 8], f);
#pragma unroll
                        for (int s_ = 0; s_ < 3; ++s_) {
                            if (c - s_ >= 0 && c - s_ < 8) {
                                float d[EPC];
                                chunk_to_f32<T>(dv[c - s_], d);
#pragma unroll
                                for (int j = 0; j < EPC; ++j) acc[rr * 3 + s_][j] += d[j] * f[j];
                            }
                        }
                    }
                }
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int j = 0; j < EPC; ++j) atomicAdd(&red[k * CHS + q * EPC + j], acc[k][j]);
    __syncthreads();
    for (int i = tid; i < 9 * CHS; i += 256) unsafeAtomicAdd(dw + (size_t)(i / CHS) * C + c0 + (i % CHS), red[i]);
}

// adjoint of the 1-D bilinear resize along one axis of a [outer][L][inner] tensor:
//   out[o][i][r] = sum_l w(l -> i) * in[o][l][r],   l over the Lout positions whose interpolation reads source i.
// IN_T / OUT_T: the side stored as T (16-byte chunks of EPC elements), the other side is f32.  Two passes (x, then y)
// give the gradient of madm_resize_bilinear with an f32 intermediate.
template <typename T, bool IN_T, bool OUT_T>
__global__ __launch_bounds__(256) void bilinear_adjoint_axis_kernel(const void* __restrict__ in_, size_t in_ld,
                                                                    void* __restrict__ out_, size_t out_ld, int outer,
                                                                    int Lout, int Lin, int inner) {
    constexpr int EPC = TT<T>::EPC;
    const unsigned G = (unsigned)inner / EPC;
    const size_t total = (size_t)outer * Lin * G;
    const float scale = (float)Lin / (float)Lout;
    const float inv = (float)Lout / (float)Lin;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const unsigned g = (unsigned)(idx % G);
        const size_t t = idx / G;
        const int i = (int)(t % (size_t)Lin);
        const size_t o = t / (size_t)Lin;
        int lo = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1;
        int hi = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1;
        if (lo < 0) lo = 0;
        if (hi > Lout - 1) hi = Lout - 1;
        float acc[EPC];
#pragma unroll
        for (int j = 0; j < EPC; ++j) acc[j] = 0.f;
        for (int l = lo; l <= hi; ++l) {
            int i0, i1;
            float l1;
            bilinear_coord(l, Lin, scale, i0, i1, l1);
            const float w = (i0 == i ? 1.f - l1 : 0.f) + (i1 == i ? l1 : 0.f);
            if (w == 0.f) continue;
            float f[EPC];
            const size_t off = (o * Lout + l) * in_ld + (size_t)g * EPC;
            if constexpr (IN_T) {
                chunk_to_f32<T>(*reinterpret_cast<const uint4*>((const T*)in_ + off), f);
            } else {
                const float* p = (const float*)in_ + off;
#pragma unroll
                for (int j = 0; j < EPC; j += 4) {
                    const float4 v = *reinterpret_cast<const float4*>(p + j);
                    f[j] = v.x; f[j + 1] = v.y; f[j + 2] = v.z; f[j + 3] = v.w;
                }
            }
#pragma unroll
            for (int j = 0; j < EPC; ++j) acc[j] += w * f[j];
        }
        const size_t ooff = (o * Lin + i) * out_ld + (size_t)g * EPC;
        if constexpr (OUT_T) {
            *reinterpret_cast<uint4*>((T*)out_ + ooff) = f32_to_chunk<T>(acc);
        } else {
            float* p = (float*)out_ + ooff;
#pragma unroll
            for (int j = 0; j < EPC; j += 4) *reinterpret_cast<float4*>(p + j) = make_float4(acc[j], acc[j + 1], acc[j + 2], acc[j + 3]);
        }
    }
}

// pixel-weighted softmax cross entropy with ignore index on f32 logit tokens [M][ldx] (K classes), one thread per pixel:
//   loss_i = w_i * (logsumexp(x_i) - x_i[label_i])   (0 where label == ignore);  loss_sum += sum_i loss_i  (f64)
//   dlogits[i][k] = coef * g * w_i * (softmax_k - [k == label_i])  (0 where ignored; columns K .. ldd-1 zero)
// CmdiseCriterion.cross_entropy (modeling/criterion.py:120-131): F.cross_entropy(reduction='none', ignore_index) *
// pixel_weight, then .mean() over ALL pixels -- the caller folds 1 / M and the loss weight into `coef`.
template <typename T>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ x, int ldx, int K,
                                                         const int64_t* __restrict__ labels,
                                                         const float* __restrict__ weight, int ignore, size_t M,
                                                         double* loss_sum, const float* __restrict__ gscale, float coef,
                                                         T* __restrict__ dlogits, int ldd) {
    __shared__ double red[4];
    double local = 0.0;
    const float g = (dlogits && gscale) ? coef * gscale[0] : coef;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < M; i += (size_t)gridDim.x * blockDim.x) {
        const float* xr = x + i * ldx;
        const long long lab = labels[i];
        const bool valid = lab != (long long)ignore && lab >= 0 && lab < K;
        const float w = valid ? (weight ? weight[i] : 1.f) : 0.f;
        float mx = xr[0];
        for (int k = 1; k < K; ++k) mx = fmaxf(mx, xr[k]);
        float se = 0.f;
        for (int k = 0; k < K; ++k) se += expf(xr[k] - mx);
        if (valid && loss_sum) local += (double)(w * (logf(se) + mx - xr[lab]));
        if (dlogits) {
            T* dr = dlogits + i * ldd;
            const float gw = g * w / se;
            for (int k = 0; k < ldd; ++k) {
                float v = 0.f;
                if (k < K && valid) v = gw * expf(xr[k] - mx) - (k == (int)lab ? g * w : 0.f);
                TT<T>::st(dr + k, v);
            }
        }
    }
    if (loss_sum) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(loss_sum, red[0] + red[1] + red[2] + red[3]);
    }
}

// masked L1 / L2 between NCHW f32 tensors pred, gt [B][C][h][w]; mask [B][Hm][Wm] is read with F.interpolate(nearest)
// to (h, w) and broadcast over C (criterion.py:236-246): loss_sum += sum |d| m  (or d^2 m);  dpred = coef g sign(d) m
// (or 2 d m)
__global__ __launch_bounds__(256) void masked_l1_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                        const float* __restrict__ mask, int B, int C, int h, int w, int Hm,
                                                        int Wm, int l2, double* loss_sum, const float* __restrict__ gscale,
                                                        float coef, float* __restrict__ dpred) {
    __shared__ double red[4];
    const size_t total = (size_t)B * C * h * w;
    const float sy = (float)Hm / (float)h, sx = (float)Wm / (float)w;
    const float g = (dpred && gscale) ? coef * gscale[0] : coef;
    double local = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xx = (int)(i % w);
        const size_t t = i / w;
        const int yy = (int)(t % h);
        const size_t b = t / h / C;
        float m = 1.f;
        if (mask) {
            int my = (int)floorf((float)yy * sy), mx = (int)floorf((float)xx * sx);
            if (my > Hm - 1) my = Hm - 1;
            if (mx > Wm - 1) mx = Wm - 1;
            m = mask[(b * Hm + my) * Wm + mx];
        }
        const float d = pred[i] - gt[i];
        if (loss_sum) local += (double)((l2 ? d * d : fabsf(d)) * m);
        if (dpred) dpred[i] = g * m * (l2 ? 2.f * d : (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f)));
    }
    if (loss_sum) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
        __syncthreads();
        if (threadIdx.x == 0) atomicAdd(loss_sum, red[0] + red[1] + red[2] + red[3]);
    }
}

// backward of tanh_gate_kernel: g_i = sum_r dout[r][i];  dx1 += tanh(a1) g;  da1 += (1 - tanh^2(a1)) x1 g;  same for 2
__global__ void tanh_gate_bwd_kernel(const float* __restrict__ a1, const float* __restrict__ x1, const float* __restrict__ a2,
                                     const float* __restrict__ x2, const float* __restrict__ dout, float* da1, float* dx1,
                                     float* da2, float* dx2, size_t n, int repeat) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float g = 0.f;
        for (int r = 0; r < repeat; ++r) g += dout[(size_t)r * n + i];
        const float t1 = a1 ? tanhf(a1[i]) : 1.f;
        if (dx1) dx1[i] += t1 * g;
        if (da1 && a1) da1[i] += (1.f - t1 * t1) * x1[i] * g;
        if (x2) {
            const float t2 = a2 ? tanhf(a2[i]) : 1.f;
            if (dx2) dx2[i] += t2 * g;
            if (da2 && a2) da2[i] += (1.f - t2 * t2) * x2[i] * g;
        }
    }
}

// train-mode BatchNorm2d bookkeeping in one launch: per-image channel sums [B][C][2] -> batch sums st [1][C][2], and the
// running statistics r = (1 - m) r + m {mean, unbiased variance} (nn.BatchNorm2d, momentum m; NULL = skip)
__global__ void bn_fold_stats_kernel(const double* __restrict__ in, int B, int C, double count, float momentum,
                                     double* __restrict__ st, float* running_mean, float* running_var) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int b = 0; b < B; ++b) {
        s += in[((size_t)b * C + c) * 2];
        q += in[((size_t)b * C + c) * 2 + 1];
    }
    st[2 * c] = s;
    st[2 * c + 1] = q;
    if (running_mean) {
        const double mean = s / count;
        double var = q / count - mean * mean;
        if (var < 0.0) var = 0.0;
        const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
        running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mean);
        running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * unb);
    }
}

// ---- colour augmentation of strong_transform (utils/dacs_transforms.py:40-78 -> kornia ColorJitter / GaussianBlur2d) ----
__device__ __forceinline__ float clamp01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }
__device__ __forceinline__ float gray_of(float r, float g, float b) { return 0.299f * r + 0.587f * g + 0.114f * b; }

// *out (f64, zeroed) += sum over pixels of the grey value of one RGB image [3][HW]
__global__ __launch_bounds__(256) void gray_sum_kernel(const float* __restrict__ img, size_t HW, double* out) {
    __shared__ double red[4];
    double local = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (size_t)gridDim.x * blockDim.x)
        local += (double)gray_of(img[i], img[HW + i], img[2 * HW + i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) local += __shfl_xor(local, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = local;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, red[0] + red[1] + red[2] + red[3]);
}

// one step of kornia's ColorJitter on one RGB image [3][HW] in [0, 1] (in place allowed):
//   op 0 brightness: x * f;  1 contrast: x * f + mean_gray * (1 - f);  2 saturation: (1 - f) * gray + f * x;
//   3 hue: rgb -> hsv, h = fmod(h + f, 2 pi), hsv -> rgb.   Ops 0-2 clamp to [0, 1].
__global__ __launch_bounds__(256) void color_jitter_kernel(const float* __restrict__ in, float* __restrict__ out, size_t HW,
                                                           int op, float f, const double* __restrict__ gray_sum) {
    const float mean = (op == 1) ? (float)(gray_sum[0] / (double)HW) : 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += (size_t)gridDim.x * blockDim.x) {
        float r = in[i], g = in[HW + i], b = in[2 * HW + i];
        if (op == 0) {
            r = clamp01(r * f); g = clamp01(g * f); b = clamp01(b * f);
        } else if (op == 1) {
            const float m = mean * (1.f - f);
            r = clamp01(r * f + m); g = clamp01(g * f + m); b = clamp01(b * f + m);
        } else if (op == 2) {
            const float y = (1.f - f) * gray_of(r, g, b);
            r = clamp01(y + f * r); g = clamp01(y + f * g); b = clamp01(y + f * b);
        } else {
            const float TWO_PI = 6.283185307179586f;
            const float mx = fmaxf(r, fmaxf(g, b)), mn = fminf(r, fminf(g, b));
            float dc = mx - mn;
            const float v = mx, s = dc / (mx + 1e-8f);
            if (dc == 0.f) dc = 1.f;
            const float rc = mx - r, gc = mx - g, bc = mx - b;
            float h = (r == mx) ? (bc - gc) : ((g == mx) ? (rc - bc) + 2.f * dc : (gc - rc) + 4.f * dc);   // first maximum wins
            h = h / dc / 6.f;
            h = h - floorf(h);                                   // python-style % 1.0
            h = fmodf(TWO_PI * h + f, TWO_PI);                   // torch.fmod keeps the sign of the dividend
            const float h6 = h / TWO_PI * 6.f;
            float hi = floorf(h6);
            hi = hi - 6.f * floorf(hi / 6.f);                    // % 6
            float ff = h6 - 6.f * floorf(h6 / 6.f) - hi;
            const float p = v * (1.f - s), q = v * (1.f - ff * s), t = v * (1.f - (1.f - ff) * s);
            const int k = (int)hi;
            r = (k == 0 || k == 5) ? v : ((k == 1) ? q : ((k == 4) ? t : p));
            g = (k == 1 || k == 2) ? v : ((k == 0) ? t : ((k == 3) ? q : p));
            b = (k == 3 || k == 4) ? v : ((k == 2) ? t : ((k == 5) ? q : p));
        }
        out[i] = r; out[HW + i] = g; out[2 * HW + i] = b;
    }
}

// 1-D correlation along x (axis 1) or y (axis 0) of `planes` f32 planes [H][W] with `ks` weights, reflect border
// (kornia filter2d_separable(border_type='reflect')).
__global__ __launch_bounds__(256) void blur_axis_kernel(const float* __restrict__ in, float* __restrict__ out, int planes,
                                                        int H, int W, int axis, int ks, const float* __restrict__ wts) {
    const size_t total = (size_t)planes * H * W;
    const int half = ks / 2, L = axis ? W : H;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const size_t t = i / W;
        const int y = (int)(t % H);
        const float* pl = in + (t / H) * (size_t)H * W;
        const int c0 = axis ? x : y;
        float acc = 0.f;
        for (int k = 0; k < ks; ++k) {
            int c = c0 + k - half;
            if (c < 0) c = -c;
            if (c >= L) c = 2 * (L - 1) - c;
            acc += wts[k] * (axis ? pl[(size_t)y * W + c] : pl[(size_t)c * W + x]);
        }
        out[i] = acc;
    }
}

// ---- masked image consistency (BlockMaskGenerator.mask_image, utils/dacs_transforms.py:136-166) ----
// Pass 1: per-block (min, max) of a flat f32 batch into part[blockIdx.x] (plain stores, no atomics and no initialisation:
// the mask kernel folds the few partials).  A NaN anywhere makes its block's pair (NaN, NaN): the reference's range tests
// are all false for a NaN minimum, so it lands in the out-of-range case.
constexpr int MIC_MAX_PARTS = 256;
__global__ __launch_bounds__(256) void mic_minmax_kernel(const float* __restrict__ x, size_t n, float2* __restrict__ part) {
    __shared__ float s_lo[4], s_hi[4];
    __shared__ int s_nan[4];
    float lo = INFINITY, hi = -INFINITY;
    bool nan = false;
    const size_t n4 = n / 4, stride = (size_t)gridDim.x * blockDim.x;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {          // four 16-byte loads in flight per thread
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = reinterpret_cast<const float4*>(x)[i + u * stride];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            nan |= (v[u].x != v[u].x) | (v[u].y != v[u].y) | (v[u].z != v[u].z) | (v[u].w != v[u].w);
            lo = fminf(fminf(lo, v[u].x), fminf(fminf(v[u].y, v[u].z), v[u].w));
            hi = fmaxf(fmaxf(hi, v[u].x), fmaxf(fmaxf(v[u].y, v[u].z), v[u].w));
        }
    }
    for (; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        nan |= (v.x != v.x) | (v.y != v.y) | (v.z != v.z) | (v.w != v.w);
        lo = fminf(fminf(lo, v.x), fminf(fminf(v.y, v.z), v.w));
        hi = fmaxf(fmaxf(hi, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float a = x[n4 * 4 + threadIdx.x];
        nan |= (a != a);
        lo = fminf(lo, a);
        hi = fmaxf(hi, a);
    }
    int bad = nan ? 1 : 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
        bad |= __shfl_xor(bad, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_lo[w] = lo; s_hi[w] = hi; s_nan[w] = bad; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < (int)(blockDim.x >> 6); ++k) { lo = fminf(lo, s_lo[k]); hi = fmaxf(hi, s_hi[k]); bad |= s_nan[k]; }
        part[blockIdx.x] = bad ? make_float2(NAN, NAN) : make_float2(lo, hi);
    }
}

// Pass 2: out = imgs with the masked 32 x 32 blocks filled.  keep(b, y, x) = u[b][gy][gx] > ratio with PyTorch's nearest
// index gy = min(floor(y * sy), gh - 1), sy = (float)gh / H (upsample_nearest2d, scales = None).  The fill is chosen on the
// device from the batch's (min, max) -- the fold of the nparts pairs of pass 1 -- in the reference's order:
//   0 <= min <= max <= 1  -> masked pixels = 0.5;   -1 <= min <= max <= 1 -> x * keep;   0 <= min <= max <= 255 -> 127.5;
//   anything else (the reference asserts) -> *flag = 1 for the host to raise on, pixels as in the 127.5 case.
// VEC consecutive pixels of one row per thread (16-byte loads / stores when W % 4 == 0).  in == out is allowed.
template <int VEC>
__global__ __launch_bounds__(256) void block_mask_kernel(const float* in, float* out, int B, int C, int H, int W,
                                                         const float* __restrict__ u, int gh, int gw, float sy, float sx,
                                                         float ratio, const float2* __restrict__ part, int nparts,
                                                         int* __restrict__ flag) {
    __shared__ float s_lo[4], s_hi[4];
    __shared__ int s_nan[4];
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int k = threadIdx.x; k < nparts; k += blockDim.x) {
        const float2 p = part[k];
        bad |= (p.x != p.x) ? 1 : 0;
        lo = fminf(lo, p.x);
        hi = fmaxf(hi, p.y);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
        bad |= __shfl_xor(bad, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_lo[w] = lo; s_hi[w] = hi; s_nan[w] = bad; }
    __syncthreads();
    for (int k = 0; k < (int)(blockDim.x >> 6); ++k) { lo = fminf(lo, s_lo[k]); hi = fmaxf(hi, s_hi[k]); bad |= s_nan[k]; }
    int mode = 3;
    if (!bad) {
        if (0.f <= lo && lo <= hi && hi <= 1.f) mode = 0;
        else if (-1.f <= lo && lo <= hi && hi <= 1.f) mode = 1;
        else if (0.f <= lo && lo <= hi && hi <= 255.f) mode = 2;
    }
    if (mode == 3 && blockIdx.x == 0 && threadIdx.x == 0) *flag = 1;
    const float fill = mode == 0 ? 0.5f : 127.5f;
    const int WV = W / VEC;
    const size_t total = (size_t)B * C * H * WV;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int xv = (int)(i % WV);
        const size_t r = i / WV;                    // row index over (b, c, y)
        const int y = (int)(r % H);
        const int b = (int)(r / ((size_t)H * C));
        const int gy = min((int)floorf((float)y * sy), gh - 1);
        const float* urow = u + ((size_t)b * gh + gy) * gw;
        float v[VEC];
        if constexpr (VEC == 4) {
            const float4 t = reinterpret_cast<const float4*>(in)[i];
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else {
            v[0] = in[i];
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const int x = xv * VEC + j;
            const int gx = min((int)floorf((float)x * sx), gw - 1);
            const bool keep = urow[gx] > ratio;
            if (mode == 1) v[j] = v[j] * (keep ? 1.f : 0.f);
            else if (!keep) v[j] = fill;
        }
        if constexpr (VEC == 4) {
            reinterpret_cast<float4*>(out)[i] = make_float4(v[0], v[1], v[2], v[3]);
        } else {
            out[i] = v[0];
        }
    }
}

unsigned grid_for(size_t n, unsigned cap = 8192) {
    size_t g = (n + 255) / 256;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

extern "C" {

int madm_scale_channels(int dtype, const void* x, int ldx, const float* scale, void* y, int ldy, int B, int HW, int C,
                        void* stream) {
    MADM_REQUIRE(x && scale && y && B > 0 && HW > 0 && C > 0, "scale_channels: bad argument");
    MADM_REQUIRE(madm_aligned16(x, y), "scale_channels: x / y must be 16-byte aligned (16-byte chunks)");
    const int epc = madm_epc(dtype);
    MADM_REQUIRE(C % epc == 0 && ldx % epc == 0 && ldy % epc == 0 && ldx >= C && ldy >= C,
                 "scale_channels: C / ld must be multiples of %d elements", epc);
    const size_t total = (size_t)B * HW * (C / epc);
    hipStream_t s = (hipStream_t)stream;
    MADM_DISPATCH_DTYPE(dtype, (scale_channels_kernel<T><<<grid_for(total), 256, 0, s>>>((const T*)x, ldx, scale, (T*)y, ldy,
                                                                                       HW, C, total)));
    return madm_check_launch("scale_channels_kernel");
}

int madm_bn_fold_stats(const double* chsums, int B, int C, double count, float momentum, double* st, float* running_mean,
                       float* running_var, void* stream) {
    MADM_REQUIRE(chsums && st && B > 0 && C > 0 && count > 0 && (!running_mean == !running_var), "bn_fold_stats: bad argument");
    bn_fold_stats_kernel<<<(C + 255) / 256, 256, 0, (hipStream_t)stream>>>(chsums, B, C, count, momentum, st, running_mean,
                                                                          running_var);
    return madm_check_launch("bn_fold_stats_kernel");
}

int madm_relu_bwd(int dtype, const void* y, const void* dy, void* dx, size_t n, void* stream) {
    MADM_REQUIRE(y && dy && dx && n > 0, "relu_bwd: bad argument");
    MADM_REQUIRE(madm_aligned16(y, dy, dx), "relu_bwd: y / dy / dx must be 16-byte aligned (16-byte chunks)");
    const int epc = madm_epc(dtype);
    MADM_REQUIRE(n % epc == 0, "relu_bwd: n must be a multiple of %d elements", epc);
    hipStream_t s = (hipStream_t)stream;
    MADM_DISPATCH_DTYPE(dtype, (relu_bwd_kernel<T><<<grid_for(n / epc), 256, 0, s>>>((const T*)y, (const T*)dy, (T*)dx,
                                                                                   n / epc)));
    return madm_check_launch("relu_bwd_kernel");
}

int madm_dwconv3x3_wgrad(int dtype, const void* x, const void* dy, int lddy, float* dw, int B, int H, int W, int C,
                         int dilation, void* stream) {
    MADM_REQUIRE(x && dy && dw && B > 0 && H > 0 && W > 0 && C > 0 && dilation > 0, "dwconv3x3_wgrad: bad argument");
    MADM_REQUIRE(madm_aligned16(x, dy), "dwconv3x3_wgrad: x / dy must be 16-byte aligned (16-byte chunks)");
    const int epc = madm_epc(dtype);
    MADM_REQUIRE(C % epc == 0 && lddy % epc == 0 && lddy >= C, "dwconv3x3_wgrad: C / lddy must be multiples of %d", epc);
    int p[6];   // variant, tile and grid: madm_dwconv3x3_plan (spatial.hip), shared with the forward
    if (const int rc = madm_dwconv3x3_plan(dtype, B, H, W, C, dilation, p, 1)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (p[0] == 4) {
        MADM_DISPATCH_DTYPE(dtype, (dwconv3x3_wgrad_lattice_kernel<T><<<(unsigned)p[5], 256, 0, s>>>(
                                       (const T*)x, (const T*)dy, lddy, dw, B, H, W, C, dilation, p[1], p[2], p[3], p[4])));
        return madm_check_launch("dwconv3x3_wgrad_lattice_kernel");
    }
    const size_t shm = (size_t)9 * C * sizeof(float);
    MADM_REQUIRE(shm <= 64 * 1024, "dwconv3x3_wgrad: C = %d too large", C);
    MADM_DISPATCH_DTYPE(dtype, (dwconv3x3_wgrad_kernel<T><<<(unsigned)p[5], 256, shm, s>>>((const T*)x, (const T*)dy, lddy, dw, B,
                                                                                         H, W, C, dilation, p[2])));
    return madm_check_launch("dwconv3x3_wgrad_kernel");
}

size_t madm_resize_bilinear_bwd_workspace_bytes(int B, int IW, int OH, int C) {
    if (B <= 0 || IW <= 0 || OH <= 0 || C <= 0) return 0;
    return (size_t)B * OH * IW * C * sizeof(float);
}

int madm_resize_bilinear_bwd(int dtype, const void* dout, int lddo, void* din, int B, int IH, int IW, int OH, int OW, int C,
                             void* workspace, size_t workspace_bytes, void* stream) {
    MADM_REQUIRE(dout && din && workspace && B > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0 && C > 0,
                 "resize_bilinear_bwd: bad argument");
    MADM_REQUIRE(madm_aligned16(dout, din, workspace), "resize_bilinear_bwd: dout / din / workspace must be 16-byte aligned (16-byte chunks)");
    const int epc = madm_epc(dtype);
    MADM_REQUIRE(C % epc == 0 && lddo % epc == 0 && lddo >= C, "resize_bilinear_bwd: C / lddo must be multiples of %d", epc);
    MADM_REQUIRE(workspace_bytes >= madm_resize_bilinear_bwd_workspace_bytes(B, IW, OH, C),
                 "resize_bilinear_bwd: workspace of %zu bytes needed", madm_resize_bilinear_bwd_workspace_bytes(B, IW, OH, C));
    hipStream_t s = (hipStream_t)stream;
    const size_t t1 = (size_t)B * OH * IW * (C / epc), t2 = (size_t)B * IH * IW * (C / epc);
    // x axis: dout [B*OH][OW][C] (row stride lddo) -> tmp f32 [B*OH][IW][C]
    MADM_DISPATCH_DTYPE(dtype, (bilinear_adjoint_axis_kernel<T, true, false><<<grid_for(t1), 256, 0, s>>>(
                                   dout, (size_t)lddo, workspace, (size_t)C, B * OH, OW, IW, C)));
    // y axis: tmp [B][OH][IW*C] -> din [B][IH][IW*C]
    MADM_DISPATCH_DTYPE(dtype, (bilinear_adjoint_axis_kernel<T, false, true><<<grid_for(t2), 256, 0, s>>>(
                                   workspace, (size_t)IW * C, din, (size_t)IW * C, B, OH, IH, IW * C)));
    return madm_check_launch("bilinear_adjoint_axis_kernel");
}

int madm_softmax_ce(int dtype, const float* logits, int ldx, int K, const int64_t* labels, const float* weight,
                    int ignore_index, size_t M, double* loss_sum, const float* gscale, float coef, void* dlogits, int ldd,
                    void* stream) {
    MADM_REQUIRE(logits && labels && M > 0 && K > 0 && ldx >= K && (loss_sum || dlogits), "softmax_ce: bad argument");
    MADM_REQUIRE(!dlogits || ldd >= K, "softmax_ce: ldd = %d < K = %d", ldd, K);
    hipStream_t s = (hipStream_t)stream;
    MADM_DISPATCH_DTYPE(dtype, (softmax_ce_kernel<T><<<grid_for(M, 4096), 256, 0, s>>>(logits, ldx, K, labels, weight,
                                                                                     ignore_index, M, loss_sum, gscale, coef,
                                                                                     (T*)dlogits, ldd)));
    return madm_check_launch("softmax_ce_kernel");
}

int madm_masked_l1(const float* pred, const float* gt, const float* mask, int B, int C, int h, int w, int Hm, int Wm, int l2,
                   double* loss_sum, const float* gscale, float coef, float* dpred, void* stream) {
    MADM_REQUIRE(pred && gt && B > 0 && C > 0 && h > 0 && w > 0 && (!mask || (Hm > 0 && Wm > 0)) && (loss_sum || dpred),
                 "masked_l1: bad argument");
    masked_l1_kernel<<<grid_for((size_t)B * C * h * w, 1024), 256, 0, (hipStream_t)stream>>>(pred, gt, mask, B, C, h, w, Hm, Wm,
                                                                                            l2, loss_sum, gscale, coef, dpred);
    return madm_check_launch("masked_l1_kernel");
}

int madm_gray_sum(const float* img, size_t HW, double* out, void* stream) {
    MADM_REQUIRE(img && out && HW > 0, "gray_sum: bad argument");
    gray_sum_kernel<<<grid_for(HW, 256), 256, 0, (hipStream_t)stream>>>(img, HW, out);
    return madm_check_launch("gray_sum_kernel");
}

int madm_color_jitter_step(const float* in, float* out, size_t HW, int op, float factor, const double* gray_sum, void* stream) {
    MADM_REQUIRE(in && out && HW > 0 && op >= 0 && op <= 3 && (op != 1 || gray_sum), "color_jitter_step: bad argument");
    color_jitter_kernel<<<grid_for(HW, 2048), 256, 0, (hipStream_t)stream>>>(in, out, HW, op, factor, gray_sum);
    return madm_check_launch("color_jitter_kernel");
}

int madm_blur_axis_f32(const float* in, float* out, int planes, int H, int W, int axis, int ksize, const float* weights,
                       void* stream) {
    MADM_REQUIRE(in && out && weights && in != out && planes > 0 && H > 0 && W > 0 && (axis == 0 || axis == 1) && ksize > 0 &&
                     ksize / 2 < (axis ? W : H), "blur_axis: bad argument");
    blur_axis_kernel<<<grid_for((size_t)planes * H * W), 256, 0, (hipStream_t)stream>>>(in, out, planes, H, W, axis, ksize, weights);
    return madm_check_launch("blur_axis_kernel");
}

int madm_tanh_gate_bwd(const float* a1, const float* x1, const float* a2, const float* x2, const float* dout, float* da1,
                       float* dx1, float* da2, float* dx2, size_t n, int repeat, void* stream) {
    MADM_REQUIRE(x1 && dout && n > 0 && repeat > 0 && (!a2 || x2), "tanh_gate_bwd: bad argument");
    tanh_gate_bwd_kernel<<<grid_for(n), 256, 0, (hipStream_t)stream>>>(a1, x1, a2, x2, dout, da1, dx1, da2, dx2, n, repeat);
    return madm_check_launch("tanh_gate_bwd_kernel");
}

int madm_mic_minmax_parts(size_t n) {
    if (n == 0) return 0;
    size_t g = (n / 4 + 1023) / 1024;      // >= 4 float4 per thread
    if (g < 1) g = 1;
    if (g > MIC_MAX_PARTS) g = MIC_MAX_PARTS;
    return (int)g;
}

int madm_mic_minmax(const float* x, size_t n, float* parts, int nparts, void* stream) {
    MADM_REQUIRE(x && parts && n > 0 && nparts == madm_mic_minmax_parts(n), "mic_minmax: bad argument");
    MADM_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)parts & 7) == 0, "mic_minmax: misaligned pointer");
    mic_minmax_kernel<<<(unsigned)nparts, 256, 0, (hipStream_t)stream>>>(x, n, reinterpret_cast<float2*>(parts));
    return madm_check_launch("mic_minmax_kernel");
}

int madm_block_mask(const float* in, float* out, int B, int C, int H, int W, const float* keep_u, int gh, int gw,
                    float scale_y, float scale_x, float mask_ratio, const float* parts, int nparts, int* flag, void* stream) {
    MADM_REQUIRE(in && out && keep_u && parts && flag && B > 0 && C > 0 && H > 0 && W > 0 && gh > 0 && gw > 0 &&
                     nparts > 0 && nparts <= MIC_MAX_PARTS,
                 "block_mask: bad argument");
    MADM_REQUIRE((in == out) || (out + (size_t)B * C * H * W <= in) || (in + (size_t)B * C * H * W <= out),
                 "block_mask: in and out overlap partially");
    // the index math of the kernel must reproduce floor(dst * scale) < src size for every dst (a bad scale would read
    // past the grid row): the clamp to gh - 1 / gw - 1 holds that, whatever the caller passes
    hipStream_t s = (hipStream_t)stream;
    const bool vec = W % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const size_t total = (size_t)B * C * H * W / (vec ? 4 : 1);
    if (vec)
        block_mask_kernel<4><<<grid_for(total, 4096), 256, 0, s>>>(in, out, B, C, H, W, keep_u, gh, gw, scale_y, scale_x,
                                                                   mask_ratio, reinterpret_cast<const float2*>(parts), nparts,
                                                                   flag);
    else
        block_mask_kernel<1><<<grid_for(total, 4096), 256, 0, s>>>(in, out, B, C, H, W, keep_u, gh, gw, scale_y, scale_x,
                                                                   mask_ratio, reinterpret_cast<const float2*>(parts), nparts,
                                                                   flag);
    return madm_check_launch("block_mask_kernel");
}

}  // extern "C"
