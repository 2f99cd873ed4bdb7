// Non-GEMM layers of the SDNet backbone / FPN on gfx950 (all HBM-bound, NHWC fp32):
// BatchNorm2d (training statistics, apply + residual + ReLU, backward), MaxPool2d(3,2,1),
// nearest-x2 upsample backward, the 1x1 head (NHWC -> NCHW) forward/backward, column sums for
// bias gradients and the fused Adam step.  They replace the torch.nn modules used by
// src/sdnet/model/network.py:6-57 and torchvision's resnet34 (BasicBlock), and
// torch.optim.Adam in src/sdnet/model/trainer.py:53,124.
#include "sd_common.h"
#include "sd_mfma.h"
#include <type_traits>

namespace sd {

// ------------------------------------------------------------------------------------------
// column reductions over a [M][C] matrix (C % 4 == 0, C <= 1024): per-block partial sums of up
// to two quantities, then a finalize kernel in double.  Thread layout: C/4 float4 columns x
// (256 / (C/4)) row lanes.
// ------------------------------------------------------------------------------------------
constexpr int RED_ROWS_PER_BLOCK = 256;

// MODE 0: sum x, sum x^2                      (BN statistics)
// MODE 1: sum g, sum g*xhat  with g = dy * [y > 0 if relu]   (BN backward)
// MODE 2: sum x                               (bias gradient)
template <int MODE, typename T = float>
__global__ __launch_bounds__(256) void k_col_reduce(const T* __restrict__ a, const T* __restrict__ b, const T* __restrict__ y,
                                                     const float* __restrict__ mean, const float* __restrict__ invstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                     int64_t M, int C, float* __restrict__ partial, int rpb) {
    __shared__ float4 red[2][256];
    const int cols = C >> 2;                       // float4 columns
    const int lanes = 256 / cols;                  // row lanes (cols <= 256)
    const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
    const int64_t r0 = (int64_t)blockIdx.x * rpb;          // rpb rows per block (red_rows(M): >= 1024 blocks where M allows)
    const int64_t r1 = min(r0 + rpb, M);
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    float4 mu = s0, is = s0, ga = s0, be = s0;
    if (MODE == 1 && rl < lanes) {
        mu = reinterpret_cast<const float4*>(mean)[col];
        is = reinterpret_cast<const float4*>(invstd)[col];
        if (relu == 2) { ga = reinterpret_cast<const float4*>(gamma)[col]; be = reinterpret_cast<const float4*>(beta)[col]; }
    }
    if (rl < lanes) {
#pragma unroll 4
        for (int64_t r = r0 + rl; r < r1; r += lanes) {
            const float4 v = ld4(a, r * cols + col);
            if (MODE == 0) {
                s0.x += v.x; s0.y += v.y; s0.z += v.z; s0.w += v.w;
                s1.x += v.x * v.x; s1.y += v.y * v.y; s1.z += v.z * v.z; s1.w += v.w * v.w;
            } else if (MODE == 2) {
                s0.x += v.x; s0.y += v.y; s0.z += v.z; s0.w += v.w;
            } else {
                float4 g = v;
                const float4 xv = ld4(b, r * cols + col);
                if (relu == 1) {            // mask from the saved post-activation (layers with a residual input)
                    const float4 yy = ld4(y, r * cols + col);
                    g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f;
                    g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
                } else if (relu == 2) {     // mask recomputed from x (same expression as k_bn_apply): one tensor read less
                    g.x = ((xv.x - mu.x) * is.x * ga.x + be.x) > 0.f ? g.x : 0.f; g.y = ((xv.y - mu.y) * is.y * ga.y + be.y) > 0.f ? g.y : 0.f;
                    g.z = ((xv.z - mu.z) * is.z * ga.z + be.z) > 0.f ? g.z : 0.f; g.w = ((xv.w - mu.w) * is.w * ga.w + be.w) > 0.f ? g.w : 0.f;
                } else if (relu == 3) {     // mask bytes written by k_bn_apply (residual layers): `y` points at them
                    const uint8_t mb = reinterpret_cast<const uint8_t*>(y)[r * cols + col];
                    g.x = (mb & 1) ? g.x : 0.f; g.y = (mb & 2) ? g.y : 0.f; g.z = (mb & 4) ? g.z : 0.f; g.w = (mb & 8) ? g.w : 0.f;
                }
                s0.x += g.x; s0.y += g.y; s0.z += g.z; s0.w += g.w;
                s1.x += g.x * ((xv.x - mu.x) * is.x); s1.y += g.y * ((xv.y - mu.y) * is.y);
                s1.z += g.z * ((xv.z - mu.z) * is.z); s1.w += g.w * ((xv.w - mu.w) * is.w);
            }
        }
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    if (rl == 0) {
        for (int l = 1; l < lanes; ++l) {
            const float4 u = red[0][l * cols + col], w = red[1][l * cols + col];
            s0.x += u.x; s0.y += u.y; s0.z += u.z; s0.w += u.w;
            s1.x += w.x; s1.y += w.y; s1.z += w.z; s1.w += w.w;
        }
        float* dst = partial + (int64_t)blockIdx.x * 2 * C;
        reinterpret_cast<float4*>(dst)[col] = s0;
        reinterpret_cast<float4*>(dst + C)[col] = s1;
    }
}

// out[j][w] = sum over the rows of slab j of in[r][w]  (W <= 1024 floats per row, W % 4 == 0): coalesced row reads
__global__ __launch_bounds__(256) void k_rows_fold(const float* __restrict__ in, int rows, int W, int slab, float* __restrict__ out) {
    __shared__ float4 red[256];
    const int cols = W >> 2, lanes = 256 / cols;
    const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
    const int r0 = blockIdx.x * slab, r1 = min(r0 + slab, rows);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rl < lanes) {
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += lanes) {
            const float4 v = reinterpret_cast<const float4*>(in + (int64_t)r * W)[col];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0) {
        for (int l = 1; l < lanes; ++l) { const float4 u = red[l * cols + col]; s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w; }
        reinterpret_cast<float4*>(out + (int64_t)blockIdx.x * W)[col] = s;
    }
}

// The per-channel double sums of the partial rows, in ONE fixed order (8-way lane tree, xor-shuffle over the 16 lanes of a wave that
// share a channel, the 4 waves through LDS): k_col_finalize and the split finish (k_col_sums + k_*_from_sums, synchronized BatchNorm)
// both reduce through it, so a split finish with no exchange in between gives today's bits.  Returns false for the lanes that own no
// result (every thread of the block must call it: it holds a barrier).
__device__ __forceinline__ bool col_pair_sums(const float* __restrict__ partial, int nblocks, int C, double (&r0)[4][4], double (&r1)[4][4],
                                              double& s0, double& s1) {
    // 4 channels x 64 lanes over the partial rows per workgroup, 8 loads in flight per lane (the pass is latency-bound: up to
    // 8192 partial rows of a few KB each); fixed order -> deterministic
    const int lc = threadIdx.x & 3, lr = threadIdx.x >> 2;
    const int c = blockIdx.x * 4 + lc;
    s0 = 0.0; s1 = 0.0;
    if (c < C) {
        double t0[8] = {0, 0, 0, 0, 0, 0, 0, 0}, t1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        // eight rows in flight per lane and trip, the last trip's missing rows read row 0 and add nothing (no serial tail: with 128-512 partial
        // rows -- most layers -- the pass used to be two to seven dependent round trips)
        for (int b = lr; b < nblocks; b += 64 * 8) {
            float v0[8], v1[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int row = b + 64 * u;
                const int64_t o = (int64_t)(row < nblocks ? row : 0) * 2 * C + c;
                v0[u] = partial[o];
                v1[u] = partial[o + C];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const bool ok = b + 64 * u < nblocks;
                t0[u] += ok ? (double)v0[u] : 0.0; t1[u] += ok ? (double)v1[u] : 0.0;
            }
        }
        s0 = ((t0[0] + t0[1]) + (t0[2] + t0[3])) + ((t0[4] + t0[5]) + (t0[6] + t0[7]));
        s1 = ((t1[0] + t1[1]) + (t1[2] + t1[3])) + ((t1[4] + t1[5]) + (t1[6] + t1[7]));
    }
    // the 16 lanes of a wave that share a channel (thread index stride 4), then the 4 waves through LDS
#pragma unroll
    for (int o = 4; o < 64; o <<= 1) { s0 += __shfl_xor(s0, o); s1 += __shfl_xor(s1, o); }
    if ((threadIdx.x & 63) < 4) { r0[threadIdx.x >> 6][lc] = s0; r1[threadIdx.x >> 6][lc] = s1; }
    __syncthreads();
    if (lr != 0 || c >= C) return false;
    s0 = (r0[0][lc] + r0[1][lc]) + (r0[2][lc] + r0[3][lc]);
    s1 = (r1[0][lc] + r1[1][lc]) + (r1[2][lc] + r1[3][lc]);
    return true;
}

// BN statistics of channel c from its sums over M elements: mean, invstd, running stats (momentum, unbiased running var)
__device__ __forceinline__ void bn_stats_tail(double s0, double s1, double M, float eps, float momentum, int c, float* __restrict__ mean_out,
                                              float* __restrict__ invstd_out, float* __restrict__ run_mean, float* __restrict__ run_var) {
    const double mean = s0 / M;
    const double var = fmax(s1 / M - mean * mean, 0.0);             // biased variance (normalisation)
    mean_out[c] = (float)mean;
    invstd_out[c] = (float)(1.0 / sqrt(var + (double)eps));
    if (run_mean) {
        const double unb = M > 1.0 ? var * M / (M - 1.0) : var;     // torch: running_var uses the unbiased estimate
        run_mean[c] = (float)((1.0 - momentum) * run_mean[c] + momentum * mean);
        run_var[c] = (float)((1.0 - momentum) * run_var[c] + momentum * unb);
    }
}

// FIN 0: BN statistics -> mean, invstd, running stats (momentum, unbiased running var)
// FIN 1: BN backward   -> dgamma (+=), dbeta (+=), and the two means needed by the apply pass
// FIN 2: bias gradient -> out0 (+=)
template <int FIN>
__global__ __launch_bounds__(256) void k_col_finalize(const float* __restrict__ partial, int nblocks, int C, double M, float eps,
                                                       float momentum, float* __restrict__ out0, float* __restrict__ out1,
                                                       float* __restrict__ run_mean, float* __restrict__ run_var,
                                                       float* __restrict__ aux0, float* __restrict__ aux1, int accumulate) {
    __shared__ double r0[4][4], r1[4][4];
    double s0, s1;
    if (!col_pair_sums(partial, nblocks, C, r0, r1, s0, s1)) return;
    const int c = blockIdx.x * 4 + (threadIdx.x & 3);
    if (FIN == 0) {
        bn_stats_tail(s0, s1, M, eps, momentum, c, out0, out1, run_mean, run_var);
    } else if (FIN == 1) {
        out0[c] = (accumulate ? out0[c] : 0.f) + (float)s1;             // dgamma = sum g * xhat
        out1[c] = (accumulate ? out1[c] : 0.f) + (float)s0;             // dbeta  = sum g
        aux0[c] = (float)(s0 / M);
        aux1[c] = (float)(s1 / M);
    } else {
        out0[c] = (accumulate ? out0[c] : 0.f) + (float)s0;
    }
}

// Split finish, phase 1 (synchronized BatchNorm): the per-channel sums of k_col_finalize, in its order, into
// sums = [S0 (C), S1 (C), n] (fp64; n = M, written by channel 0's lane).  FIN 1 also writes dgamma / dbeta from these LOCAL sums.
template <int FIN>
__global__ __launch_bounds__(256) void k_col_sums(const float* __restrict__ partial, int nblocks, int C, double M, float* __restrict__ dgamma,
                                                   float* __restrict__ dbeta, int accumulate, double* __restrict__ sums) {
    __shared__ double r0[4][4], r1[4][4];
    double s0, s1;
    if (!col_pair_sums(partial, nblocks, C, r0, r1, s0, s1)) return;
    const int c = blockIdx.x * 4 + (threadIdx.x & 3);
    sums[c] = s0;
    sums[C + c] = s1;
    if (c == 0) sums[2 * C] = M;
    if (FIN == 1) {
        dgamma[c] = (accumulate ? dgamma[c] : 0.f) + (float)s1;
        dbeta[c] = (accumulate ? dbeta[c] : 0.f) + (float)s0;
    }
}

// Split finish, phase 2 of the forward: mean, invstd and the running statistics from (possibly all-reduced) sums -- the tail of
// k_col_finalize<0> with n = sums[2C]
__global__ __launch_bounds__(256) void k_bn_stats_from_sums(const double* __restrict__ sums, int C, float eps, float momentum,
                                                             float* __restrict__ mean, float* __restrict__ invstd,
                                                             float* __restrict__ run_mean, float* __restrict__ run_var) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    bn_stats_tail(sums[c], sums[C + c], sums[2 * C], eps, momentum, c, mean, invstd, run_mean, run_var);
}

// Split finish, phase 2 of the backward: means = [mean(g) (C), mean(g * xhat) (C)] for the apply pass, n = sums[2C]
__global__ __launch_bounds__(256) void k_bn_bwd_means_from_sums(const double* __restrict__ sums, int C, float* __restrict__ means) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const double M = sums[2 * C];
    means[c] = (float)(sums[c] / M);
    means[C + c] = (float)(sums[C + c] / M);
}

// y = [relu]( (x - mean) * invstd * gamma + beta [+ res] )
template <typename T>
__global__ __launch_bounds__(256) void k_bn_apply(const T* __restrict__ x, T* __restrict__ y, int64_t n4, int C,
                                                   const float* __restrict__ mean, const float* __restrict__ invstd,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   const T* __restrict__ res, int relu, uint8_t* __restrict__ mask) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int cols = C >> 2;
    // The grid stride is a multiple of the column count for every power-of-two channel count (256 % cols == 0): a thread then stays on
    // ONE column and its four parameter vectors are loaded once -- inside the loop they were four 16-byte L1 requests next to one or two
    // requests of data per element (`fixed`); other channel counts take the per-element lookup.
    const bool fixed = stride % cols == 0;
    const int col0 = (int)(((int64_t)blockIdx.x * 256 + threadIdx.x) % cols);
    float4 mu = reinterpret_cast<const float4*>(mean)[col0], is = reinterpret_cast<const float4*>(invstd)[col0];
    float4 g = reinterpret_cast<const float4*>(gamma)[col0], b = reinterpret_cast<const float4*>(beta)[col0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 v = ld4(x, i);
        if (!fixed) {
            const int col = (int)(i % cols);
            mu = reinterpret_cast<const float4*>(mean)[col]; is = reinterpret_cast<const float4*>(invstd)[col];
            g = reinterpret_cast<const float4*>(gamma)[col]; b = reinterpret_cast<const float4*>(beta)[col];
        }
        float4 o;
        o.x = (v.x - mu.x) * is.x * g.x + b.x; o.y = (v.y - mu.y) * is.y * g.y + b.y;
        o.z = (v.z - mu.z) * is.z * g.z + b.z; o.w = (v.w - mu.w) * is.w * g.w + b.w;
        if (res) {
            const float4 r = ld4(res, i);
            o.x += r.x; o.y += r.y; o.z += r.z; o.w += r.w;
        }
        // one mask byte per float4 (bit j = element j is positive): the backward of a residual layer reads 1/16 of the bytes of y
        if (mask) mask[i] = (uint8_t)((o.x > 0.f ? 1 : 0) | (o.y > 0.f ? 2 : 0) | (o.z > 0.f ? 4 : 0) | (o.w > 0.f ? 8 : 0));
        if (relu) { o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f); }
        st4(y, i, o);
    }
}

// eval-mode BN folded into a per-channel affine (consumed by the conv epilogue)
__global__ __launch_bounds__(256) void k_bn_fold(const float* gamma, const float* beta, const float* rm, const float* rv, float eps,
                                                  int C, float* scale, float* shift) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    const float s = gamma[c] / sqrtf(rv[c] + eps);
    scale[c] = s;
    shift[c] = beta[c] - rm[c] * s;
}

// dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * [y > 0];  optionally g_out = g
template <typename T>
__global__ __launch_bounds__(256) void k_bn_bwd_apply(const T* __restrict__ dy, const T* __restrict__ x, const T* __restrict__ y,
                                                       int relu, int64_t n4, int C, const float* __restrict__ mean,
                                                       const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ mg,
                                                       const float* __restrict__ mgx, T* __restrict__ dx, T* __restrict__ g_out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int cols = C >> 2;
    const bool fixed = stride % cols == 0;                      // (see k_bn_apply: one column per thread, parameters loaded once)
    const int col0 = (int)(((int64_t)blockIdx.x * 256 + threadIdx.x) % cols);
    float4 mu = reinterpret_cast<const float4*>(mean)[col0], is = reinterpret_cast<const float4*>(invstd)[col0];
    float4 ga = reinterpret_cast<const float4*>(gamma)[col0];
    float4 be = relu == 2 ? reinterpret_cast<const float4*>(beta)[col0] : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 a = reinterpret_cast<const float4*>(mg)[col0], b = reinterpret_cast<const float4*>(mgx)[col0];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 g = ld4(dy, i);
        const float4 xv = ld4(x, i);
        if (!fixed) {
            const int col = (int)(i % cols);
            mu = reinterpret_cast<const float4*>(mean)[col]; is = reinterpret_cast<const float4*>(invstd)[col];
            ga = reinterpret_cast<const float4*>(gamma)[col];
            if (relu == 2) be = reinterpret_cast<const float4*>(beta)[col];
            a = reinterpret_cast<const float4*>(mg)[col]; b = reinterpret_cast<const float4*>(mgx)[col];
        }
        if (relu == 1) {
            const float4 yy = ld4(y, i);
            g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f; g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
        } else if (relu == 3) {
            const uint8_t mb = reinterpret_cast<const uint8_t*>(y)[i];
            g.x = (mb & 1) ? g.x : 0.f; g.y = (mb & 2) ? g.y : 0.f; g.z = (mb & 4) ? g.z : 0.f; g.w = (mb & 8) ? g.w : 0.f;
        } else if (relu == 2) {
            g.x = ((xv.x - mu.x) * is.x * ga.x + be.x) > 0.f ? g.x : 0.f; g.y = ((xv.y - mu.y) * is.y * ga.y + be.y) > 0.f ? g.y : 0.f;
            g.z = ((xv.z - mu.z) * is.z * ga.z + be.z) > 0.f ? g.z : 0.f; g.w = ((xv.w - mu.w) * is.w * ga.w + be.w) > 0.f ? g.w : 0.f;
        }
        float4 o;
        o.x = ga.x * is.x * (g.x - a.x - (xv.x - mu.x) * is.x * b.x);
        o.y = ga.y * is.y * (g.y - a.y - (xv.y - mu.y) * is.y * b.y);
        o.z = ga.z * is.z * (g.z - a.z - (xv.z - mu.z) * is.z * b.z);
        o.w = ga.w * is.w * (g.w - a.w - (xv.w - mu.w) * is.w * b.w);
        st4(dx, i, o);
        if (g_out) st4(g_out, i, g);
    }
}

// MaxPool2d(3, stride 2, pad 1), NHWC.  idx = winning tap (first maximum in row-major window
// order, as ATen) for the backward.
__global__ __launch_bounds__(256) void k_maxpool_fwd(const float* __restrict__ x, float* __restrict__ y, uint8_t* __restrict__ idx, int B,
                                                      int Hi, int Wi, int Ho, int Wo, int C) {
    const int cols = C >> 2;
    const int64_t n4 = (int64_t)B * Ho * Wo * cols;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int col = (int)(i % cols);
    int64_t t = i / cols;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    uchar4 w = make_uchar4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int iy = oy * 2 - 1 + r, ix = ox * 2 - 1 + s;
            if (iy < 0 || iy >= Hi || ix < 0 || ix >= Wi) continue;
            const float4 v = reinterpret_cast<const float4*>(x + (((int64_t)b * Hi + iy) * Wi + ix) * C)[col];
            const uint8_t tap = (uint8_t)(r * 3 + s);
            if (v.x > m.x) { m.x = v.x; w.x = tap; }
            if (v.y > m.y) { m.y = v.y; w.y = tap; }
            if (v.z > m.z) { m.z = v.z; w.z = tap; }
            if (v.w > m.w) { m.w = v.w; w.w = tap; }
        }
    }
    reinterpret_cast<float4*>(y)[i] = m;
    reinterpret_cast<uchar4*>(idx)[i] = w;
}

// gather form of the max-pool backward (no atomics): every input pixel looks at the <= 4 windows
// that contain it.
__global__ __launch_bounds__(256) void k_maxpool_bwd(const float* __restrict__ dy, const uint8_t* __restrict__ idx, float* __restrict__ dx,
                                                      int B, int Hi, int Wi, int Ho, int Wo, int C) {
    const int cols = C >> 2;
    const int64_t n4 = (int64_t)B * Hi * Wi * cols;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int col = (int)(i % cols);
    int64_t t = i / cols;
    const int ix = (int)(t % Wi); t /= Wi;
    const int iy = (int)(t % Hi);
    const int b = (int)(t / Hi);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = (iy + 1) / 2 - ((iy + 1) % 2 == 0 ? 1 : 0); oy <= (iy + 1) / 2; ++oy) {
        if (oy < 0 || oy >= Ho) continue;
        const int r = iy - (oy * 2 - 1);
        if (r < 0 || r > 2) continue;
        for (int ox = (ix + 1) / 2 - ((ix + 1) % 2 == 0 ? 1 : 0); ox <= (ix + 1) / 2; ++ox) {
            if (ox < 0 || ox >= Wo) continue;
            const int s = ix - (ox * 2 - 1);
            if (s < 0 || s > 2) continue;
            const int64_t o = (((int64_t)b * Ho + oy) * Wo + ox) * cols + col;
            const uchar4 w = reinterpret_cast<const uchar4*>(idx)[o];
            const float4 g = reinterpret_cast<const float4*>(dy)[o];
            const uint8_t tap = (uint8_t)(r * 3 + s);
            if (w.x == tap) acc.x += g.x;
            if (w.y == tap) acc.y += g.y;
            if (w.z == tap) acc.z += g.z;
            if (w.w == tap) acc.w += g.w;
        }
    }
    reinterpret_cast<float4*>(dx)[i] = acc;
}

// ---- stem tail fused: BatchNorm(train) + ReLU + MaxPool2d(3, 2, 1) without materialising the full-resolution activation.
// forward: the pooled map and the winning taps straight from the conv output x (same affine expression as k_bn_apply, same
// first-maximum rule as k_maxpool_fwd).
// XT / PT: element type of the conv output x and of the pooled map (float, or uint16_t = bf16 in the mixed-precision step: fp32 arithmetic,
// one rounding at the store; the winning tap is decided on the fp32 values)
template <typename XT, typename PT>
__global__ __launch_bounds__(256) void k_bn_relu_maxpool_fwd(const XT* __restrict__ x, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, PT* __restrict__ y,
                                                              uint8_t* __restrict__ idx, int B, int Hi, int Wi, int Ho, int Wo, int C) {
    const int cols = C >> 2;
    const int64_t n4 = (int64_t)B * Ho * Wo * cols;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int col = (int)(i % cols);
    int64_t t = i / cols;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    const float4 mu = reinterpret_cast<const float4*>(mean)[col], is = reinterpret_cast<const float4*>(invstd)[col];
    const float4 ga = reinterpret_cast<const float4*>(gamma)[col], be = reinterpret_cast<const float4*>(beta)[col];
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    uchar4 w = make_uchar4(0, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int iy = oy * 2 - 1 + r, ix = ox * 2 - 1 + s;
            if (iy < 0 || iy >= Hi || ix < 0 || ix >= Wi) continue;
            const float4 xv = ld4(x, (((int64_t)b * Hi + iy) * Wi + ix) * cols + col);
            float4 v;
            v.x = fmaxf((xv.x - mu.x) * is.x * ga.x + be.x, 0.f); v.y = fmaxf((xv.y - mu.y) * is.y * ga.y + be.y, 0.f);
            v.z = fmaxf((xv.z - mu.z) * is.z * ga.z + be.z, 0.f); v.w = fmaxf((xv.w - mu.w) * is.w * ga.w + be.w, 0.f);
            const uint8_t tap = (uint8_t)(r * 3 + s);
            if (v.x > m.x) { m.x = v.x; w.x = tap; }
            if (v.y > m.y) { m.y = v.y; w.y = tap; }
            if (v.z > m.z) { m.z = v.z; w.z = tap; }
            if (v.w > m.w) { m.w = v.w; w.w = tap; }
        }
    }
    st4(y, i, m);
    reinterpret_cast<uchar4*>(idx)[i] = w;
}

// The same pass, two horizontally adjacent windows per thread (Wo even) and 16 bytes per load for both element types (fp32: 4 channels,
// bf16: 8): the windows (oy, 2 j) and (oy, 2 j + 1) share the input column 4 j + 1, so 15 loads serve two outputs (7.5 per output; the
// one-window form needs 9, of 8 bytes for bf16: 258 us at bs = 64 for a 140 us floor).  Same affine expression, same scan order
// (row-major, strict >): the same winning taps.  Plain loads: every input element is read by two or four threads.
template <int VEC> struct PoolVec { float v[VEC]; };
__device__ __forceinline__ PoolVec<4> pool_ld(const float* p, int64_t e) {
    const float4 r = *reinterpret_cast<const float4*>(p + e);
    return PoolVec<4>{{r.x, r.y, r.z, r.w}};
}
__device__ __forceinline__ PoolVec<8> pool_ld(const uint16_t* p, int64_t e) {
    const uint4 r = *reinterpret_cast<const uint4*>(p + e);
    return PoolVec<8>{{bf16_to_f32((uint16_t)(r.x & 0xffff)), bf16_to_f32((uint16_t)(r.x >> 16)), bf16_to_f32((uint16_t)(r.y & 0xffff)), bf16_to_f32((uint16_t)(r.y >> 16)),
                       bf16_to_f32((uint16_t)(r.z & 0xffff)), bf16_to_f32((uint16_t)(r.z >> 16)), bf16_to_f32((uint16_t)(r.w & 0xffff)), bf16_to_f32((uint16_t)(r.w >> 16))}};
}
__device__ __forceinline__ void pool_st(float* p, int64_t e, const PoolVec<4>& m) { *reinterpret_cast<float4*>(p + e) = make_float4(m.v[0], m.v[1], m.v[2], m.v[3]); }
__device__ __forceinline__ void pool_st(uint16_t* p, int64_t e, const PoolVec<8>& m) {
    uint4 r;
    r.x = (uint32_t)f32_to_bf16(m.v[0]) | ((uint32_t)f32_to_bf16(m.v[1]) << 16); r.y = (uint32_t)f32_to_bf16(m.v[2]) | ((uint32_t)f32_to_bf16(m.v[3]) << 16);
    r.z = (uint32_t)f32_to_bf16(m.v[4]) | ((uint32_t)f32_to_bf16(m.v[5]) << 16); r.w = (uint32_t)f32_to_bf16(m.v[6]) | ((uint32_t)f32_to_bf16(m.v[7]) << 16);
    *reinterpret_cast<uint4*>(p + e) = r;
}
template <typename XT, typename PT, int VEC>
__global__ __launch_bounds__(256) void k_bn_relu_maxpool_fwd_pair(const XT* __restrict__ x, const float* __restrict__ mean,
                                                                   const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, PT* __restrict__ y,
                                                                   uint8_t* __restrict__ idx, int B, int Hi, int Wi, int Ho, int Wo, int C) {
    const int cols = C / VEC, Wp = Wo >> 1;
    const int64_t n = (int64_t)B * Ho * Wp * cols;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int col = (int)(i % cols);
    int64_t t = i / cols;
    const int oxp = (int)(t % Wp); t /= Wp;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    float mu[VEC], is[VEC], ga[VEC], be[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { mu[k] = mean[col * VEC + k]; is[k] = invstd[col * VEC + k]; ga[k] = gamma[col * VEC + k]; be[k] = beta[col * VEC + k]; }
    PoolVec<VEC> m0, m1;
    uint8_t w0[VEC], w1[VEC];
#pragma unroll
    for (int k = 0; k < VEC; ++k) { m0.v[k] = m1.v[k] = -INFINITY; w0[k] = w1[k] = 0; }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int iy = oy * 2 - 1 + r;
        if (iy < 0 || iy >= Hi) continue;
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            const int ix = oxp * 4 - 1 + c;
            if (ix < 0 || ix >= Wi) continue;
            const PoolVec<VEC> xv = pool_ld(x, (((int64_t)b * Hi + iy) * Wi + ix) * C + col * VEC);
#pragma unroll
            for (int k = 0; k < VEC; ++k) {
                const float v = fmaxf((xv.v[k] - mu[k]) * is[k] * ga[k] + be[k], 0.f);
                if (c <= 2 && v > m0.v[k]) { m0.v[k] = v; w0[k] = (uint8_t)(r * 3 + c); }
                if (c >= 2 && v > m1.v[k]) { m1.v[k] = v; w1[k] = (uint8_t)(r * 3 + c - 2); }
            }
        }
    }
    const int64_t o = (((int64_t)b * Ho + oy) * Wo + 2 * oxp) * C + col * VEC;
    pool_st(y, o, m0); pool_st(y, o + C, m1);
    uint32_t p0[VEC / 4], p1[VEC / 4];
#pragma unroll
    for (int k = 0; k < VEC / 4; ++k) {
        p0[k] = w0[4 * k] | ((uint32_t)w0[4 * k + 1] << 8) | ((uint32_t)w0[4 * k + 2] << 16) | ((uint32_t)w0[4 * k + 3] << 24);
        p1[k] = w1[4 * k] | ((uint32_t)w1[4 * k + 1] << 8) | ((uint32_t)w1[4 * k + 2] << 16) | ((uint32_t)w1[4 * k + 3] << 24);
    }
#pragma unroll
    for (int k = 0; k < VEC / 4; ++k) { reinterpret_cast<uint32_t*>(idx + o)[k] = p0[k]; reinterpret_cast<uint32_t*>(idx + o + C)[k] = p1[k]; }
}

// gradient w.r.t. the (never stored) BatchNorm+ReLU output at input pixel (b, iy, ix): gather form of the max-pool backward
// (k_maxpool_bwd) followed by the ReLU mask recomputed from x
__device__ __forceinline__ float4 pool_relu_grad(const float* __restrict__ dpool, const uint8_t* __restrict__ idx, int b, int iy, int ix,
                                                 int col, int cols, int Ho, int Wo, const float4 xv, const float4 mu, const float4 is,
                                                 const float4 ga, const float4 be) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int oy = (iy + 1) / 2 - ((iy + 1) % 2 == 0 ? 1 : 0); oy <= (iy + 1) / 2; ++oy) {
        if (oy < 0 || oy >= Ho) continue;
        const int r = iy - (oy * 2 - 1);
        if (r < 0 || r > 2) continue;
        for (int ox = (ix + 1) / 2 - ((ix + 1) % 2 == 0 ? 1 : 0); ox <= (ix + 1) / 2; ++ox) {
            if (ox < 0 || ox >= Wo) continue;
            const int s = ix - (ox * 2 - 1);
            if (s < 0 || s > 2) continue;
            const int64_t o = (((int64_t)b * Ho + oy) * Wo + ox) * cols + col;
            const uchar4 w = reinterpret_cast<const uchar4*>(idx)[o];
            const float4 g = reinterpret_cast<const float4*>(dpool)[o];
            const uint8_t tap = (uint8_t)(r * 3 + s);
            if (w.x == tap) acc.x += g.x;
            if (w.y == tap) acc.y += g.y;
            if (w.z == tap) acc.z += g.z;
            if (w.w == tap) acc.w += g.w;
        }
    }
    acc.x = ((xv.x - mu.x) * is.x * ga.x + be.x) > 0.f ? acc.x : 0.f; acc.y = ((xv.y - mu.y) * is.y * ga.y + be.y) > 0.f ? acc.y : 0.f;
    acc.z = ((xv.z - mu.z) * is.z * ga.z + be.z) > 0.f ? acc.z : 0.f; acc.w = ((xv.w - mu.w) * is.w * ga.w + be.w) > 0.f ? acc.w : 0.f;
    return acc;
}

// The same gradient for the four pixels (2k + dy, 2j + dx) of an even-aligned 2x2 quad at once (Hi, Wi even): they only see the
// windows (k, j), (k, j+1), (k+1, j), (k+1, j+1), so four window loads serve four pixels (the per-pixel gather needs nine) and
// the window set is fixed -- no data-dependent loops.  g[2 * dy + dx].
template <typename PT>
__device__ __forceinline__ void pool_relu_grad_quad(const PT* __restrict__ dpool, const uint8_t* __restrict__ idx, int b, int k, int j,
                                                    int col, int cols, int Ho, int Wo, const float4* xv, const float4 mu, const float4 is,
                                                    const float4 ga, const float4 be, float4* g) {
    const bool hy = k + 1 < Ho, hx = j + 1 < Wo;
    const int64_t o00 = (((int64_t)b * Ho + k) * Wo + j) * cols + col;
    const int64_t o01 = hx ? o00 + cols : o00, o10 = hy ? o00 + (int64_t)Wo * cols : o00, o11 = (hx && hy) ? o00 + (int64_t)(Wo + 1) * cols : o00;
    const uchar4 w00 = reinterpret_cast<const uchar4*>(idx)[o00], w01 = reinterpret_cast<const uchar4*>(idx)[o01];
    const uchar4 w10 = reinterpret_cast<const uchar4*>(idx)[o10], w11 = reinterpret_cast<const uchar4*>(idx)[o11];
    const float4 d00 = ld4(dpool, o00);
    float4 d01 = ld4(dpool, o01), d10 = ld4(dpool, o10);
    float4 d11 = ld4(dpool, o11);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    if (!hx) d01 = z;
    if (!hy) d10 = z;
    if (!(hx && hy)) d11 = z;
#define SD_PICK(W, D, TAP) make_float4((W).x == (TAP) ? (D).x : 0.f, (W).y == (TAP) ? (D).y : 0.f, (W).z == (TAP) ? (D).z : 0.f, (W).w == (TAP) ? (D).w : 0.f)
#define SD_ADD4(A, B) { (A).x += (B).x; (A).y += (B).y; (A).z += (B).z; (A).w += (B).w; }
    // pixel (2k, 2j): window (k, j) tap (1, 1)
    g[0] = SD_PICK(w00, d00, 4);
    // pixel (2k, 2j+1): (k, j) tap (1, 2); (k, j+1) tap (1, 0)
    g[1] = SD_PICK(w00, d00, 5); { const float4 t = SD_PICK(w01, d01, 3); SD_ADD4(g[1], t) }
    // pixel (2k+1, 2j): (k, j) tap (2, 1); (k+1, j) tap (0, 1)
    g[2] = SD_PICK(w00, d00, 7); { const float4 t = SD_PICK(w10, d10, 1); SD_ADD4(g[2], t) }
    // pixel (2k+1, 2j+1): (k, j) tap (2, 2); (k, j+1) tap (2, 0); (k+1, j) tap (0, 2); (k+1, j+1) tap (0, 0)
    g[3] = SD_PICK(w00, d00, 8);
    { const float4 t = SD_PICK(w01, d01, 6); SD_ADD4(g[3], t) }
    { const float4 t = SD_PICK(w10, d10, 2); SD_ADD4(g[3], t) }
    { const float4 t = SD_PICK(w11, d11, 0); SD_ADD4(g[3], t) }
#undef SD_PICK
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        g[q].x = ((xv[q].x - mu.x) * is.x * ga.x + be.x) > 0.f ? g[q].x : 0.f; g[q].y = ((xv[q].y - mu.y) * is.y * ga.y + be.y) > 0.f ? g[q].y : 0.f;
        g[q].z = ((xv[q].z - mu.z) * is.z * ga.z + be.z) > 0.f ? g[q].z : 0.f; g[q].w = ((xv[q].w - mu.w) * is.w * ga.w + be.w) > 0.f ? g[q].w : 0.f;
    }
}

// quad form of the reduction pass: a block takes RED_ROWS_PER_BLOCK / 4 quads (same partial-row count as the pixel form)
template <typename XT, typename PT>
__global__ __launch_bounds__(256) void k_pool_bn_bwd_reduce_quad(const PT* __restrict__ dpool, const uint8_t* __restrict__ idx,
                                                                  const XT* __restrict__ x, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, int Hi, int Wi, int Ho, int Wo, int64_t MQ,
                                                                  int C, float* __restrict__ partial) {
    __shared__ float4 red[2][256];
    const int cols = C >> 2, lanes = 256 / cols;
    const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
    constexpr int QPB = RED_ROWS_PER_BLOCK / 4;
    const int64_t q0 = (int64_t)blockIdx.x * QPB, q1 = min(q0 + QPB, MQ);
    const int Hq = Hi >> 1, Wq = Wi >> 1;
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    if (rl < lanes) {
        const float4 mu = reinterpret_cast<const float4*>(mean)[col], is = reinterpret_cast<const float4*>(invstd)[col];
        const float4 ga = reinterpret_cast<const float4*>(gamma)[col], be = reinterpret_cast<const float4*>(beta)[col];
        for (int64_t q = q0 + rl; q < q1; q += lanes) {
            const int j = (int)(q % Wq);
            const int64_t t = q / Wq;
            const int k = (int)(t % Hq), b = (int)(t / Hq);
            const int64_t p00 = (((int64_t)b * Hi + 2 * k) * Wi + 2 * j) * cols + col;
            float4 xv[4], g[4];
            xv[0] = ld4(x, p00); xv[1] = ld4(x, p00 + cols);
            xv[2] = ld4(x, p00 + (int64_t)Wi * cols); xv[3] = ld4(x, p00 + (int64_t)(Wi + 1) * cols);
            pool_relu_grad_quad(dpool, idx, b, k, j, col, cols, Ho, Wo, xv, mu, is, ga, be, g);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s0.x += g[u].x; s0.y += g[u].y; s0.z += g[u].z; s0.w += g[u].w;
                s1.x += g[u].x * ((xv[u].x - mu.x) * is.x); s1.y += g[u].y * ((xv[u].y - mu.y) * is.y);
                s1.z += g[u].z * ((xv[u].z - mu.z) * is.z); s1.w += g[u].w * ((xv[u].w - mu.w) * is.w);
            }
        }
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    if (rl == 0) {
        for (int l = 1; l < lanes; ++l) {
            const float4 u = red[0][l * cols + col], w = red[1][l * cols + col];
            s0.x += u.x; s0.y += u.y; s0.z += u.z; s0.w += u.w;
            s1.x += w.x; s1.y += w.y; s1.z += w.z; s1.w += w.w;
        }
        float* dst = partial + (int64_t)blockIdx.x * 2 * C;
        reinterpret_cast<float4*>(dst)[col] = s0;
        reinterpret_cast<float4*>(dst + C)[col] = s1;
    }
}

template <typename XT, typename PT, typename DT = float>
__global__ __launch_bounds__(256) void k_pool_bn_bwd_apply_quad(const PT* __restrict__ dpool, const uint8_t* __restrict__ idx,
                                                                 const XT* __restrict__ x, const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ mg,
                                                                 const float* __restrict__ mgx, int Hi, int Wi, int Ho, int Wo, int64_t nq4,
                                                                 int C, DT* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nq4) return;
    const int cols = C >> 2;
    const int col = (int)(i % cols);
    const int64_t q = i / cols;
    const int Hq = Hi >> 1, Wq = Wi >> 1;
    const int j = (int)(q % Wq);
    const int64_t t = q / Wq;
    const int k = (int)(t % Hq), b = (int)(t / Hq);
    const float4 mu = reinterpret_cast<const float4*>(mean)[col], is = reinterpret_cast<const float4*>(invstd)[col];
    const float4 ga = reinterpret_cast<const float4*>(gamma)[col], be = reinterpret_cast<const float4*>(beta)[col];
    const float4 a = reinterpret_cast<const float4*>(mg)[col], bb = reinterpret_cast<const float4*>(mgx)[col];
    const int64_t p00 = (((int64_t)b * Hi + 2 * k) * Wi + 2 * j) * cols + col;
    const int64_t off[4] = {p00, p00 + cols, p00 + (int64_t)Wi * cols, p00 + (int64_t)(Wi + 1) * cols};
    float4 xv[4], g[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) xv[u] = ld4(x, off[u]);
    pool_relu_grad_quad(dpool, idx, b, k, j, col, cols, Ho, Wo, xv, mu, is, ga, be, g);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        float4 o;
        o.x = ga.x * is.x * (g[u].x - a.x - (xv[u].x - mu.x) * is.x * bb.x);
        o.y = ga.y * is.y * (g[u].y - a.y - (xv[u].y - mu.y) * is.y * bb.y);
        o.z = ga.z * is.z * (g[u].z - a.z - (xv[u].z - mu.z) * is.z * bb.z);
        o.w = ga.w * is.w * (g[u].w - a.w - (xv[u].w - mu.w) * is.w * bb.w);
        st4(dx, off[u], o);
    }
}
#undef SD_ADD4

// reduction pass of the fused backward: per-channel partial sums of g and g * xhat over RED_ROWS_PER_BLOCK pixels (layout as k_col_reduce)
__global__ __launch_bounds__(256) void k_pool_bn_bwd_reduce(const float* __restrict__ dpool, const uint8_t* __restrict__ idx,
                                                             const float* __restrict__ x, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, int Hi, int Wi, int Ho, int Wo, int64_t M,
                                                             int C, float* __restrict__ partial) {
    __shared__ float4 red[2][256];
    const int cols = C >> 2, lanes = 256 / cols;
    const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
    const int64_t r0 = (int64_t)blockIdx.x * RED_ROWS_PER_BLOCK, r1 = min(r0 + RED_ROWS_PER_BLOCK, M);
    float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
    if (rl < lanes) {
        const float4 mu = reinterpret_cast<const float4*>(mean)[col], is = reinterpret_cast<const float4*>(invstd)[col];
        const float4 ga = reinterpret_cast<const float4*>(gamma)[col], be = reinterpret_cast<const float4*>(beta)[col];
        for (int64_t r = r0 + rl; r < r1; r += lanes) {
            const int ix = (int)(r % Wi);
            const int64_t t = r / Wi;
            const int iy = (int)(t % Hi), b = (int)(t / Hi);
            const float4 xv = reinterpret_cast<const float4*>(x + r * C)[col];
            const float4 g = pool_relu_grad(dpool, idx, b, iy, ix, col, cols, Ho, Wo, xv, mu, is, ga, be);
            s0.x += g.x; s0.y += g.y; s0.z += g.z; s0.w += g.w;
            s1.x += g.x * ((xv.x - mu.x) * is.x); s1.y += g.y * ((xv.y - mu.y) * is.y);
            s1.z += g.z * ((xv.z - mu.z) * is.z); s1.w += g.w * ((xv.w - mu.w) * is.w);
        }
    }
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    if (rl == 0) {
        for (int l = 1; l < lanes; ++l) {
            const float4 u = red[0][l * cols + col], w = red[1][l * cols + col];
            s0.x += u.x; s0.y += u.y; s0.z += u.z; s0.w += u.w;
            s1.x += w.x; s1.y += w.y; s1.z += w.z; s1.w += w.w;
        }
        float* dst = partial + (int64_t)blockIdx.x * 2 * C;
        reinterpret_cast<float4*>(dst)[col] = s0;
        reinterpret_cast<float4*>(dst + C)[col] = s1;
    }
}

// apply pass of the fused backward: dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat))
__global__ __launch_bounds__(256) void k_pool_bn_bwd_apply(const float* __restrict__ dpool, const uint8_t* __restrict__ idx,
                                                            const float* __restrict__ x, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mg,
                                                            const float* __restrict__ mgx, int Hi, int Wi, int Ho, int Wo, int64_t n4, int C,
                                                            float* __restrict__ dx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int cols = C >> 2;
    const int col = (int)(i % cols);
    const int64_t r = i / cols;
    const int ix = (int)(r % Wi);
    const int64_t t = r / Wi;
    const int iy = (int)(t % Hi), b = (int)(t / Hi);
    const float4 mu = reinterpret_cast<const float4*>(mean)[col], is = reinterpret_cast<const float4*>(invstd)[col];
    const float4 ga = reinterpret_cast<const float4*>(gamma)[col], be = reinterpret_cast<const float4*>(beta)[col];
    const float4 xv = reinterpret_cast<const float4*>(x)[i];
    const float4 g = pool_relu_grad(dpool, idx, b, iy, ix, col, cols, Ho, Wo, xv, mu, is, ga, be);
    const float4 a = reinterpret_cast<const float4*>(mg)[col], bb = reinterpret_cast<const float4*>(mgx)[col];
    float4 o;
    o.x = ga.x * is.x * (g.x - a.x - (xv.x - mu.x) * is.x * bb.x);
    o.y = ga.y * is.y * (g.y - a.y - (xv.y - mu.y) * is.y * bb.y);
    o.z = ga.z * is.z * (g.z - a.z - (xv.z - mu.z) * is.z * bb.z);
    o.w = ga.w * is.w * (g.w - a.w - (xv.w - mu.w) * is.w * bb.w);
    reinterpret_cast<float4*>(dx)[i] = o;
}

// backward of nearest x2 upsample: dx[b,y,x,c] = sum of the 2x2 block of dy (+ add, nullable)
template <typename T>
__global__ __launch_bounds__(256) void k_up2_bwd(const T* __restrict__ dy, const T* __restrict__ add, T* __restrict__ dx, int B,
                                                  int H, int W, int C) {
    const int cols = C >> 2;
    const int64_t n4 = (int64_t)B * H * W * cols;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n4) return;
    const int col = (int)(i % cols);
    int64_t t = i / cols;
    const int x = (int)(t % W); t /= W;
    const int y = (int)(t % H);
    const int b = (int)(t / H);
    const T* base = dy + (((int64_t)b * 2 * H + 2 * y) * 2 * W + 2 * x) * C;
    const float4 v0 = ld4(base, col), v1 = ld4(base + C, col);
    const float4 v2 = ld4(base + (int64_t)2 * W * C, col);
    const float4 v3 = ld4(base + (int64_t)2 * W * C + C, col);
    float4 o = make_float4(v0.x + v1.x + v2.x + v3.x, v0.y + v1.y + v2.y + v3.y, v0.z + v1.z + v2.z + v3.z, v0.w + v1.w + v2.w + v3.w);
    if (add) {
        const float4 a = ld4(add, i);
        o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
    }
    st4(dx, i, o);
}

// ------------------------------------------------------------------------------------------
// Head: 1x1 conv C -> Co (<= 16) with bias, NHWC in, NCHW out (network.py:22-29,57).
// 64 pixels per block: the [64][C] tile is one contiguous 64*C*4-byte span, staged in LDS with a
// 4-float row pad (ds_read_b128 conflict-free), then thread (pixel, group) accumulates its
// outputs with wave-uniform (broadcast) weight reads.  HBM-bound: AI ~ 3 flop/B.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_head_fwd(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ y, int64_t M, int HW, int C, int Co) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = C + 4;
    float* xs = lds;                 // [64][C+4]
    float* ws = lds + 64 * LD;       // [Co][C]
    const int64_t m0 = (int64_t)blockIdx.x * 64;
    const int c4 = C >> 2;
    for (int i = threadIdx.x; i < 64 * c4; i += 256) {
        const int row = i / c4, col = i - row * c4;
        const int64_t m = m0 + row;
        const float4 v = m < M ? reinterpret_cast<const float4*>(x + m * C)[col] : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(xs + row * LD + col * 4) = v;
    }
    for (int i = threadIdx.x; i < Co * C; i += 256) ws[i] = w[i];
    __syncthreads();
    const int px = threadIdx.x & 63, grp = threadIdx.x >> 6;
    float acc[HEAD_NARROW_MAX_CO / 4];
#pragma unroll
    for (int j = 0; j < HEAD_NARROW_MAX_CO / 4; ++j) acc[j] = 0.f;
    for (int c = 0; c < C; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(xs + px * LD + c);
#pragma unroll
        for (int j = 0; j < HEAD_NARROW_MAX_CO / 4; ++j) {
            const int co = grp + 4 * j;
            if (co < Co) {
                const float4 ww = *reinterpret_cast<const float4*>(ws + co * C + c);
                acc[j] += v.x * ww.x + v.y * ww.y + v.z * ww.z + v.w * ww.w;
            }
        }
    }
    const int64_t m = m0 + px;
    if (m < M) {
        const int64_t b = m / HW, pix = m - b * HW;
#pragma unroll
        for (int j = 0; j < HEAD_NARROW_MAX_CO / 4; ++j) {
            const int co = grp + 4 * j;
            if (co < Co) y[(b * Co + co) * HW + pix] = acc[j] + bias[co];
        }
    }
}

// Head forward on an fp32 NHWC input of 128 channels (the default FPN depth), Co <= 16: 537 MB in, 29 MB out at bs = 64 -- a pure HBM
// stream.  k_head_fwd above stages 64 pixels per block and re-reads every staged row once per output-channel group plus the weights
// per thread (13x the input bytes in LDS reads): 230 us, twice the stream's time.  Here, as in k_head_fwd_bf16_c128, every WAVE walks
// its own tiles of 16 pixels with a private ring of NST stages (8 KB each) filled by LDS-DMA NST - 1 tiles ahead (no staging registers,
// no block barrier, counted vmcnt), and multiplies on v_mfma_f32_16x16x4_f32: A = the tile (lane (row, kq) reads chunk 4 j + kq of its
// pixel: one ds_read_b128 per four MFMA steps), B = the weights in registers (lane (n, kq): w[n][16 j + 4 kq + t]), D = 16 pixels x 16
// output channels, lane (n, q) holding pixels 4 q .. 4 q + 3 of channel n: one 16-byte store into the NCHW plane.
//   LDS image of a tile: row r x 32 slots of 16 bytes, chunk c of row r at physical slot c ^ (r & 15) (swizzle applied to the DMA's
//   SOURCE address; the 16 lanes of a ds_read_b128 pass -- rows 0 .. 15, same chunk -- hit 16 different slots).
constexpr int HF_NST = 4;
__global__ __launch_bounds__(256) void k_head_fwd_f32_c128(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ y, int HW, int Co, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) float hf_lds[];             // 4 waves x HF_NST x 8 KB
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* const T = hf_lds + wave * (HF_NST * 2048);
    const uint32_t t_base = lds_addr(T);
    const int row = lane & 15, kq = lane >> 4;
    f32x4 bw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        bw[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row < Co) bw[j] = *reinterpret_cast<const f32x4*>(w + row * 128 + 16 * j + 4 * kq);
    }
    const float bv = row < Co ? bias[row] : 0.f;
    const int nwaves = gridDim.x * 4;
    const int dr = lane >> 5, dsl = lane & 31;                                 // DMA: lane -> (row within a 2-row piece, physical slot)
    // tile t -> ring stage st: eight 1 KB pieces; tiles past the end re-read the last tile (the vmcnt accounting stays fixed; never consumed)
#define HF_ISSUE(t_, st_)                                                                                          \
    {                                                                                                              \
        const int64_t m0_ = (int64_t)min((t_), ntiles - 1) * 16;                                                  \
        _Pragma("unroll") for (int d = 0; d < 8; ++d) {                                                            \
            const int r = 2 * d + dr;                                                                              \
            lds_dma16(x + (m0_ + r) * 128 + ((dsl ^ (r & 15)) << 2), T + (st_) * 2048 + d * 256);                   \
        }                                                                                                          \
    }
    int tile = blockIdx.x * 4 + wave;
#pragma unroll
    for (int s = 0; s < HF_NST - 1; ++s) HF_ISSUE(tile + s * nwaves, s)
    int stage = 0;
    for (; tile < ntiles; tile += nwaves) {
        const int nst = stage == 0 ? HF_NST - 1 : stage - 1;                   // the stage consumed in the previous trip (its reads were waited for)
        HF_ISSUE(tile + (HF_NST - 1) * nwaves, nst)
        // at most the pieces of the HF_NST - 1 younger tiles outstanding (this wave's interleaved output stores only make the wait stricter)
        wait_vmcnt<8 * (HF_NST - 1)>();
        const uint32_t a0 = t_base + (uint32_t)stage * 8192u + (uint32_t)row * 512u;
        f32x4 a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = lds_read128_async<0>(a0 + (uint32_t)(((4 * j + kq) ^ row) << 4));
        SD_LDS_WAIT4(0, a[0], a[1], a[2], a[3]);
        SD_LDS_WAIT4(0, a[4], a[5], a[6], a[7]);
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 8; j += 2)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j][t], bw[j][t], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[j + 1][t], bw[j + 1][t], acc1, 0, 0, 0);
            }
        if (row < Co) {
            const uint32_t m0 = (uint32_t)tile * 16u;                          // (M < 2^31)
            const uint32_t b = m0 / (uint32_t)HW, pix = m0 - b * (uint32_t)HW; // (HW % 16 == 0: a tile stays inside one image)
            const f32x4 o = {acc0[0] + acc1[0] + bv, acc0[1] + acc1[1] + bv, acc0[2] + acc1[2] + bv, acc0[3] + acc1[3] + bv};
            *reinterpret_cast<f32x4*>(y + ((int64_t)b * Co + row) * HW + pix + 4 * kq) = o;
        }
        stage = stage + 1 == HF_NST ? 0 : stage + 1;
    }
    wait_vmcnt<0>();                                                           // (past-the-end DMAs still landing in this wave's LDS)
#undef HF_ISSUE
}

// head data-gradient: dx[m][c] = sum_co dy[b][co][pix] * w[co][c]   (NCHW grad in, NHWC out)
constexpr int HEAD_WG_PIX = 1024;   // pixels per block of the head weight-gradient kernels
template <typename T>      // T = float, or uint16_t: dx is stored as bf16 (mixed-precision training)
__global__ __launch_bounds__(256) void k_head_dgrad(const float* __restrict__ dy, const float* __restrict__ w, T* __restrict__ dx,
                                                     int64_t M, int HW, int C, int Co) {
    __shared__ float gs[HEAD_NARROW_MAX_CO][64];
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* ws = lds;                 // [Co][C]
    const int64_t m0 = (int64_t)blockIdx.x * 64;
    for (int i = threadIdx.x; i < Co * 64; i += 256) {
        const int co = i >> 6, px = i & 63;
        const int64_t m = m0 + px;
        float v = 0.f;
        if (m < M) { const int64_t b = m / HW, pix = m - b * HW; v = dy[(b * Co + co) * HW + pix]; }
        gs[co][px] = v;
    }
    for (int i = threadIdx.x; i < Co * C; i += 256) ws[i] = w[i];
    __syncthreads();
    const int c4 = C >> 2;
    for (int i = threadIdx.x; i < 64 * c4; i += 256) {
        const int row = i / c4, col = i - row * c4;
        const int64_t m = m0 + row;
        if (m >= M) continue;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int co = 0; co < Co; ++co) {
            const float g = gs[co][row];
            const float4 ww = *reinterpret_cast<const float4*>(ws + co * C + col * 4);
            o.x += g * ww.x; o.y += g * ww.y; o.z += g * ww.z; o.w += g * ww.w;
        }
        if constexpr (sizeof(T) == 2) {
            uint2 pk;
            pk.x = (uint32_t)f32_to_bf16(o.x) | ((uint32_t)f32_to_bf16(o.y) << 16);
            pk.y = (uint32_t)f32_to_bf16(o.z) | ((uint32_t)f32_to_bf16(o.w) << 16);
            reinterpret_cast<uint2*>(dx + m * C)[col] = pk;
        } else {
            reinterpret_cast<float4*>(dx + m * C)[col] = o;
        }
    }
}

// head weight / bias gradient partials from a bf16 NHWC activation (mixed precision): a thread owns 8 consecutive channels (one 16-byte
// load per pixel: a wave-instruction reads 1 KB contiguous) and every 256 / (C / 8)-th pixel of a 64-pixel chunk, CO x 8 fp32 sums in
// registers; the pixel lanes are combined by wave shuffles and through LDS in a fixed order.  Same partial layout as k_head_wgrad.
template <int CO>
__global__ __launch_bounds__(256) void k_head_wgrad_bf16(const float* __restrict__ dy, const uint16_t* __restrict__ x, float* __restrict__ partial,
                                                          int64_t M, int HW, int C, int Co) {
    __shared__ float gs[CO][64];
    __shared__ float comb[4][CO * 128];               // per wave: [co][c] (C <= 128 here)
    const int64_t mb = (int64_t)blockIdx.x * HEAD_WG_PIX;
    const int CG = C >> 3, PL = 256 / CG;             // channel groups, pixel lanes (C = 128: 16 x 16; C = 64: 8 x 32)
    const int cg = threadIdx.x % CG, pl = threadIdx.x / CG;
    float acc[CO][8];
#pragma unroll
    for (int j = 0; j < CO; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[j][k] = 0.f;
    float bsum = 0.f;
    for (int64_t m0 = mb; m0 < min(mb + HEAD_WG_PIX, M); m0 += 64) {
        __syncthreads();
        for (int i = threadIdx.x; i < Co * 64; i += 256) {
            const int co = i >> 6, px = i & 63;
            const int64_t m = m0 + px;
            float v = 0.f;
            if (m < M) { const int64_t b = m / HW, pix = m - b * HW; v = dy[(b * Co + co) * HW + pix]; }
            gs[co][px] = v;
        }
        __syncthreads();
        for (int p0 = 0; p0 < 64; p0 += 4 * PL) {      // four 16-byte loads in flight per thread
            uint4 xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int px = p0 + u * PL + pl;
                const int64_t m = m0 + px;
                xv[u] = reinterpret_cast<const uint4*>(x + (px < 64 && m < M ? m : mb) * C)[cg];      // masked rows meet gs == 0 (or are skipped below)
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int px = p0 + u * PL + pl;
                if (px >= 64) continue;
                const float f[8] = {__uint_as_float(xv[u].x << 16), __uint_as_float(xv[u].x & 0xffff0000u), __uint_as_float(xv[u].y << 16),
                                    __uint_as_float(xv[u].y & 0xffff0000u), __uint_as_float(xv[u].z << 16), __uint_as_float(xv[u].z & 0xffff0000u),
                                    __uint_as_float(xv[u].w << 16), __uint_as_float(xv[u].w & 0xffff0000u)};
#pragma unroll
                for (int j = 0; j < CO; ++j) {
                    if (j < Co) {
                        const float g = gs[j][px];
#pragma unroll
                        for (int k = 0; k < 8; ++k) acc[j][k] += g * f[k];
                    }
                }
            }
        }
        if (threadIdx.x < Co) {
            for (int px = 0; px < 64; ++px) bsum += gs[threadIdx.x][px];
        }
    }
    // pixel lanes of one wave (lanes with the same cg: stride CG), then the four waves in order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < CO; ++j)
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            float v = acc[j][k];
            for (int o = CG; o < 64; o <<= 1) v += __shfl_xor(v, o);
            acc[j][k] = v;
        }
    if (lane < CG) {
#pragma unroll
        for (int j = 0; j < CO; ++j)
            if (j < Co) {
#pragma unroll
                for (int k = 0; k < 8; ++k) comb[wave][j * C + lane * 8 + k] = acc[j][k];
            }
    }
    __syncthreads();
    float* dst = partial + (int64_t)blockIdx.x * (Co * C + Co);
    for (int i = threadIdx.x; i < Co * C; i += 256) dst[i] = (comb[0][i] + comb[1][i]) + (comb[2][i] + comb[3][i]);
    if (threadIdx.x < Co) dst[Co * C + threadIdx.x] = bsum;
}

// head weight/bias gradient partials: block handles HEAD_WG_PIX pixels in 64-pixel chunks; thread (c, half)
// accumulates Co sums over its half of every chunk (all 256 threads busy when C == 128), 8 loads in flight.
__global__ __launch_bounds__(256) void k_head_wgrad(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
                                                     int64_t M, int HW, int C, int Co) {
    __shared__ float gs[HEAD_NARROW_MAX_CO][64];
    __shared__ float comb[HEAD_NARROW_MAX_CO][256];
    const int64_t mb = (int64_t)blockIdx.x * HEAD_WG_PIX;
    const int halves = max(1, 256 / C);                 // pixel sub-ranges handled in parallel
    const int c = threadIdx.x % C, hf = threadIdx.x / C;
    const int span = 64 / halves;
    float acc[HEAD_NARROW_MAX_CO];
#pragma unroll
    for (int j = 0; j < HEAD_NARROW_MAX_CO; ++j) acc[j] = 0.f;
    float bsum = 0.f;                                   // thread co < Co also accumulates the bias gradient
    for (int64_t m0 = mb; m0 < min(mb + HEAD_WG_PIX, M); m0 += 64) {
        __syncthreads();
        for (int i = threadIdx.x; i < Co * 64; i += 256) {
            const int co = i >> 6, px = i & 63;
            const int64_t m = m0 + px;
            float v = 0.f;
            if (m < M) { const int64_t b = m / HW, pix = m - b * HW; v = dy[(b * Co + co) * HW + pix]; }
            gs[co][px] = v;
        }
        __syncthreads();
        if (hf < halves) {
            const int p0 = hf * span;
#pragma unroll 1
            for (int pb = 0; pb < span; pb += 8) {
                float xv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int64_t m = m0 + p0 + pb + u;
                    xv[u] = x[(m < M ? m : mb) * C + c];          // unconditional load; masked rows have gs == 0
                }
#pragma unroll
                for (int u = 0; u < 8; ++u)
#pragma unroll
                    for (int j = 0; j < HEAD_NARROW_MAX_CO; ++j)
                        if (j < Co) acc[j] += gs[j][p0 + pb + u] * xv[u];
            }
        }
        if (threadIdx.x < Co) {
            for (int px = 0; px < 64; ++px) bsum += gs[threadIdx.x][px];
        }
    }
    // combine the pixel halves
    for (int j = 0; j < Co; ++j) comb[j][threadIdx.x] = (hf < halves) ? acc[j] : 0.f;
    __syncthreads();
    float* dst = partial + (int64_t)blockIdx.x * (Co * C + Co);
    if (threadIdx.x < C) {
        for (int j = 0; j < Co; ++j) {
            float t = 0.f;
            for (int h2 = 0; h2 < halves; ++h2) t += comb[j][h2 * C + threadIdx.x];
            dst[j * C + threadIdx.x] = t;
        }
    }
    if (threadIdx.x < Co) dst[Co * C + threadIdx.x] = bsum;
}

// Head weight / bias gradient partials from an fp32 NHWC activation of 128 channels, Co <= 16, on v_mfma_f32_16x16x4_f32 (the reduction
// index of the MFMA is the PIXEL).  Same wave-private LDS-DMA ring as k_head_fwd_f32_c128 (tiles of 16 pixels, HF_NST stages, eight 1 KB
// pieces of x per tile, swizzled on the source side) plus one piece for dy: lane (co = n, kq) fetches dy[co][pixels 4 kq .. 4 kq + 3]
// from the NCHW plane into its own 16-byte slot.  Per tile: A = dy (one ds_read_b128 per lane), B = x: lane (n, kq) reads chunks n and
// 16 + n of pixels 4 kq + i (channels {4 n .. 4 n + 3, 64 + 4 n .. 64 + 4 n + 3}: 8 ds_read_b128, conflict-free), 32 MFMAs; x is read
// exactly once (537 MB at bs = 64).  k_head_wgrad (scalar loads, LDS-broadcast dy, 7 FMAs per loaded float): 343 us, 3x the stream's time.
// One partial row per WAVE, same layout as k_head_wgrad's (finished by k_head_wgrad_fin in a fixed order).
constexpr int HWG_STAGE = 2048 + 256;                                          // floats: 8 KB of x + 1 KB of dy
__global__ __launch_bounds__(256) void k_head_wgrad_f32_c128(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
                                                              int HW, int Co, int ntiles) {
    extern __shared__ __attribute__((aligned(16))) float hw_lds[];             // 4 waves x HF_NST x 9 KB
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* const T = hw_lds + wave * (HF_NST * HWG_STAGE);
    const uint32_t t_base = lds_addr(T);
    const int n = lane & 15, kq = lane >> 4;
    const int gw = blockIdx.x * 4 + wave, nwaves = gridDim.x * 4;
    const int dr = lane >> 5, dsl = lane & 31;
    const int nco = min(n, Co - 1);                                            // (lanes n >= Co fetch a valid plane; their A operand is zeroed)
#define HWG_ISSUE(t_, st_)                                                                                         \
    {                                                                                                              \
        const uint32_t m0_ = (uint32_t)min((t_), ntiles - 1) * 16u;                      /* (M < 2^31) */        \
        const uint32_t b_ = m0_ / (uint32_t)HW, pix_ = m0_ - b_ * (uint32_t)HW;                                     \
        _Pragma("unroll") for (int d = 0; d < 8; ++d) {                                                            \
            const int r = 2 * d + dr;                                                                              \
            lds_dma16(x + ((int64_t)m0_ + r) * 128 + ((dsl ^ (r & 15)) << 2), T + (st_) * HWG_STAGE + d * 256);     \
        }                                                                                                          \
        lds_dma16(dy + ((int64_t)b_ * Co + nco) * HW + pix_ + 4 * kq, T + (st_) * HWG_STAGE + 2048);               \
    }
    f32x4 acc[8];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) acc[cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    float bsum = 0.f;
    int tile = gw;
#pragma unroll
    for (int s = 0; s < HF_NST - 1; ++s) HWG_ISSUE(tile + s * nwaves, s)
    int stage = 0;
    for (; tile < ntiles; tile += nwaves) {
        const int nst = stage == 0 ? HF_NST - 1 : stage - 1;
        HWG_ISSUE(tile + (HF_NST - 1) * nwaves, nst)
        wait_vmcnt<9 * (HF_NST - 1)>();
        const uint32_t s0 = t_base + (uint32_t)stage * (HWG_STAGE * 4);
        f32x4 a = lds_read128_async<0>(s0 + 8192u + (uint32_t)lane * 16u);
        f32x4 xa[4], xb[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t row = (uint32_t)(4 * kq + i);
            xa[i] = lds_read128_async<0>(s0 + row * 512u + (((uint32_t)n ^ (row & 15u)) << 4));
            xb[i] = lds_read128_async<0>(s0 + row * 512u + (((uint32_t)(16 + n) ^ (row & 15u)) << 4));
        }
        SD_LDS_WAIT4(0, xa[0], xa[1], xa[2], xa[3]);
        SD_LDS_WAIT4(0, xb[0], xb[1], xb[2], xb[3]);
        SD_LDS_WAIT2(0, a, xa[0]);
        if (n >= Co) a = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                acc[cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], xa[i][cb], acc[cb], 0, 0, 0);
                acc[4 + cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], xb[i][cb], acc[4 + cb], 0, 0, 0);
            }
        bsum += (a[0] + a[1]) + (a[2] + a[3]);
        stage = stage + 1 == HF_NST ? 0 : stage + 1;
    }
    wait_vmcnt<0>();
#undef HWG_ISSUE
    // D: lane (n' = n, q = kq) holds dW[co = 4 q + r][channel(n', cb)], channel = 4 n' + cb (cb < 4), 64 + 4 n' + cb - 4 (cb >= 4)
    float* dst = partial + (int64_t)gw * (Co * 128 + Co);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int co = 4 * kq + r;
        if (co < Co) {                                                         // (row length Co * 129: no 16-byte alignment -> scalar stores)
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) { dst[co * 128 + 4 * n + cb] = acc[cb][r]; dst[co * 128 + 64 + 4 * n + cb] = acc[4 + cb][r]; }
        }
    }
    bsum += __shfl_xor(bsum, 16);
    bsum += __shfl_xor(bsum, 32);
    if (kq == 0 && n < Co) dst[Co * 128 + n] = bsum;
}

// 8 outputs x 32 lanes over the partial blocks per workgroup (deterministic order)
__global__ __launch_bounds__(256) void k_head_wgrad_fin(const float* __restrict__ partial, int nblocks, int n, float* __restrict__ dw,
                                                         float* __restrict__ db, int nw, int accumulate) {
    __shared__ double red[32][8];
    const int lo = threadIdx.x & 7, lr = threadIdx.x >> 3;
    const int i = blockIdx.x * 8 + lo;
    double s = 0.0;
    if (i < n)
        for (int b = lr; b < nblocks; b += 32) s += (double)partial[(int64_t)b * n + i];
    red[lr][lo] = s;
    __syncthreads();
    if (lr != 0 || i >= n) return;
    for (int k = 1; k < 32; ++k) s += red[k][lo];
    float* dst = i < nw ? dw + i : db + (i - nw);
    *dst = (accumulate ? *dst : 0.f) + (float)s;
}

// ------------------------------------------------------------------------------------------
// Adam (torch.optim.Adam defaults: no weight decay, no amsgrad), one launch over the flat
// parameter buffer.  612 MB of traffic per step for 21.85 M parameters: HBM-bound.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                               float* __restrict__ v, int64_t n4, float lr, float b1, float b2, float eps, float bc1,
                                               float bc2_sqrt, float gscale) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float* P = &pp.x; const float* G = &gg.x; float* Mo = &mm.x; float* V = &vv.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gr = G[j] * gscale;
            Mo[j] = b1 * Mo[j] + (1.f - b1) * gr;                     // exp_avg.lerp_(grad, 1 - beta1)
            V[j] = b2 * V[j] + (1.f - b2) * gr * gr;                  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
            const float denom = sqrtf(V[j]) / bc2_sqrt + eps;
            P[j] -= (lr / bc1) * (Mo[j] / denom);
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
    }
}

// ------------------------------------------------------------------------------------------
// Optimizer step with options (sd_optim_step): decoupled weight decay (torch.optim.AdamW), global-norm
// clipping (torch.nn.utils.clip_grad_norm_) and a weight EMA, fused into k_adam's one pass.  The norm
// needs every gradient before the first update: k_grad_sumsq leaves one fp64 partial per block and
// every block of k_optim finishes them itself (at most 4 KB from L2) -- no third launch, no host trip.
// Both reductions run in a fixed order (per thread in index order, 64 lanes by shuffle, 4 waves in
// order): the same gradients give the same bits on every run and every rank.  No atomics.
// ------------------------------------------------------------------------------------------
constexpr int SUMSQ_MAX_BLOCKS = 512;         // partials: 2 blocks per CU, eight 16-byte loads in flight per thread

__device__ __forceinline__ double sumsq4(const float4 a) {
    return ((double)a.x * a.x + (double)a.y * a.y) + ((double)a.z * a.z + (double)a.w * a.w);
}

// sum of 256 per-thread doubles, the same value in every thread
__device__ __forceinline__ double block_sum_256(double s, double* red4) {
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red4[0] + red4[1]) + red4[2]) + red4[3];
}

// (plain loads, not non-temporal ones: the update kernel that follows re-reads the same 87 MB, which may then still be in the last-level cache)
__global__ __launch_bounds__(256) void k_grad_sumsq(const float* __restrict__ g, int64_t n4, double* __restrict__ partial) {
    __shared__ double red[4];
    const int64_t stride = (int64_t)gridDim.x * 256;
    const float4* G = reinterpret_cast<const float4*>(g);
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += 8 * stride) {
        float4 a[8];                                       // eight loads in flight; past the end: the last group re-read, counted as zero
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = G[min(i + k * stride, n4 - 1)];
#pragma unroll
        for (int k = 0; k < 8; ++k) s += i + k * stride < n4 ? sumsq4(a[k]) : 0.0;
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// status block (SD_OPTIM_STATUS_BYTES): [0] float global norm, [1] float clip coefficient, [2] int32 skipped steps, [3] reserved
template <bool DECAY, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_optim(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, int64_t n4, float lr, float b1, float b2, float eps, float bc1,
                                                float bc2_sqrt, float gscale, float decay_mul, const uint8_t* __restrict__ mask,
                                                float max_norm, const double* __restrict__ partial, int npartial,
                                                float* __restrict__ ema, float ema_decay, uint32_t* __restrict__ status) {
    float coef = 1.f;
    if (CLIP) {
        __shared__ double red[4];
        double s = 0.0;
        for (int k = threadIdx.x; k < npartial; k += 256) s += partial[k];
        s = block_sum_256(s, red);
        const float norm = (float)(fabs((double)gscale) * sqrt(s));            // of the gradient after grad_scale
        const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
        coef = finite ? fminf(1.f, max_norm / (norm + 1e-6f)) : 0.f;           // clip_grad_norm_: max_norm / (total_norm + 1e-6), clamped to 1
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            status[0] = __float_as_uint(norm);
            status[1] = __float_as_uint(coef);
            if (!finite) status[2] = status[2] + 1u;
        }
        if (!finite) return;                                                   // an inf / nan gradient: the step is skipped, nothing is written
    }
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float4 ee = make_float4(0.f, 0.f, 0.f, 0.f);
        if (EMA) ee = reinterpret_cast<float4*>(ema)[i];
        const bool decay = DECAY && (mask == nullptr || mask[i] != 0);
        float* P = &pp.x; const float* G = &gg.x; float* Mo = &mm.x; float* V = &vv.x; float* E = &ee.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gr = G[j] * gscale;
            if (CLIP) gr *= coef;
            if (decay) P[j] *= decay_mul;                            // AdamW: param.mul_(1 - lr * weight_decay)
            Mo[j] = b1 * Mo[j] + (1.f - b1) * gr;                     // from here on: k_adam, same operation order
            V[j] = b2 * V[j] + (1.f - b2) * gr * gr;
            const float denom = sqrtf(V[j]) / bc2_sqrt + eps;
            P[j] -= (lr / bc1) * (Mo[j] / denom);
            if (EMA) E[j] = ema_decay * E[j] + (1.f - ema_decay) * P[j];
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (EMA) reinterpret_cast<float4*>(ema)[i] = ee;
    }
}

// The same pass with a learning rate and a decay per parameter group (sd_optim_groups_step): one id byte per group of four floats, laid
// out like k_optim's mask, names a row of a table of SD_OPTIM_MAX_GROUPS rows that arrives by value in the kernel arguments (SGPRs).
// Every lane keeps row (lane & 15) of it in two registers, and a group's row is fetched from lane (id & 15) by a wave shuffle (two
// ds_bpermute a float4) -- registers only: no table in memory, so no load that depends on the id byte -- and everything behind the pick
// is k_optim's body in k_optim's order.  `decay_bits` bit k: group k is decayed at all (the multiply by
// decay_mul stays behind a condition, as in k_optim, so that both kernels round alike); a row past ngroups is lr 0 / no decay.
struct OptimGroupTable {
    float step[SD_OPTIM_MAX_GROUPS];           // lr_k / bc1 with lr_k = lr * lr_mul[k]: k_optim's `lr / bc1`, the same fp32 division done on the host
    float decay_mul[SD_OPTIM_MAX_GROUPS];      // 1 - lr_k * weight_decay * wd_mul[k]
};

template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_optim_groups(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, int64_t n4, const OptimGroupTable tab, uint32_t decay_bits, float b1,
                                                       float b2, float eps, float bc2_sqrt, float gscale,
                                                       const uint8_t* __restrict__ ids, float max_norm, const double* __restrict__ partial,
                                                       int npartial, float* __restrict__ ema, float ema_decay, uint32_t* __restrict__ status) {
    float coef = 1.f;
    if (CLIP) {                                                                // k_optim's finish of the partials, word for word
        __shared__ double red[4];
        double s = 0.0;
        for (int k = threadIdx.x; k < npartial; k += 256) s += partial[k];
        s = block_sum_256(s, red);
        const float norm = (float)(fabs((double)gscale) * sqrt(s));
        const bool finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
        coef = finite ? fminf(1.f, max_norm / (norm + 1e-6f)) : 0.f;
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            status[0] = __float_as_uint(norm);
            status[1] = __float_as_uint(coef);
            if (!finite) status[2] = status[2] + 1u;
        }
        if (!finite) return;                                                   // skipped for every group
    }
    // the table, once per thread: lane l of a wave keeps row l & 15 in two registers
    const uint32_t lane = threadIdx.x & 63u, row = lane & (SD_OPTIM_MAX_GROUPS - 1u);
    float row_step = tab.step[0], row_decay_mul = tab.decay_mul[0];
#pragma unroll
    for (uint32_t q = 1; q < SD_OPTIM_MAX_GROUPS; ++q) {
        row_step = row == q ? tab.step[q] : row_step;
        row_decay_mul = row == q ? tab.decay_mul[q] : row_decay_mul;
    }
    const int64_t stride = (int64_t)gridDim.x * 256;
    // the loop runs per WAVE (its bound is the wave's first group), so that the whole wave is live at the shuffles: a lane past the end
    // takes part in them and skips the rest
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); base < n4; base += stride) {
        const int64_t i = base + lane;
        const bool live = i < n4;
        const uint32_t k = live ? ids[i] & (SD_OPTIM_MAX_GROUPS - 1u) : 0u;    // a stray byte names a row of the table, never memory
        const float step = __shfl(row_step, (int)k), decay_mul = __shfl(row_decay_mul, (int)k);   // lane k (< 16) holds row k
        if (!live) continue;
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
        float4 ee = make_float4(0.f, 0.f, 0.f, 0.f);
        if (EMA) ee = reinterpret_cast<float4*>(ema)[i];
        const bool decay = (decay_bits >> k & 1u) != 0;
        float* P = &pp.x; const float* G = &gg.x; float* Mo = &mm.x; float* V = &vv.x; float* E = &ee.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gr = G[j] * gscale;
            if (CLIP) gr *= coef;
            if (decay) P[j] *= decay_mul;
            Mo[j] = b1 * Mo[j] + (1.f - b1) * gr;
            V[j] = b2 * V[j] + (1.f - b2) * gr * gr;
            const float denom = sqrtf(V[j]) / bc2_sqrt + eps;
            P[j] -= step * (Mo[j] / denom);
            if (EMA) E[j] = ema_decay * E[j] + (1.f - ema_decay) * P[j];
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        reinterpret_cast<float4*>(m)[i] = mm;
        reinterpret_cast<float4*>(v)[i] = vv;
        if (EMA) reinterpret_cast<float4*>(ema)[i] = ee;
    }
}

// ------------------------------------------------------------------------------------------
// The other two update rules over the same flat buffers, both in the groups form (id byte per group of four, rates and decays by value):
// SGD with momentum (sd_sgd_step, torch.optim.SGD with dampening 0) and LAMB (sd_lamb_step, You et al. 2020, Alg. 2).
// ------------------------------------------------------------------------------------------
// k_optim's finish of the sd_grad_sumsq partials: the norm, the coefficient, and whether the step runs at all.  `writer`: this thread
// records them in the status block (one thread of one launch of a step).
__device__ __forceinline__ float clip_coef_256(const double* __restrict__ partial, int npartial, float gscale, float max_norm, double* red4,
                                               uint32_t* __restrict__ status, bool writer, bool& finite) {
    double s = 0.0;
    for (int k = threadIdx.x; k < npartial; k += 256) s += partial[k];
    s = block_sum_256(s, red4);
    const float norm = (float)(fabs((double)gscale) * sqrt(s));
    finite = (__float_as_uint(norm) & 0x7f800000u) != 0x7f800000u;
    const float coef = finite ? fminf(1.f, max_norm / (norm + 1e-6f)) : 0.f;
    if (writer) {
        status[0] = __float_as_uint(norm);
        status[1] = __float_as_uint(coef);
        if (!finite) status[2] = status[2] + 1u;
    }
    return coef;
}

struct SgdGroupTable {
    float lr[SD_OPTIM_MAX_GROUPS];             // lr * lr_mul[k]
    float wd[SD_OPTIM_MAX_GROUPS];             // weight_decay * wd_mul[k]; 0: the group is not decayed
};

// SGD: k_optim_groups's pass (the table in registers, picked by a wave shuffle) with one state buffer, or none.
// MOM 0: no momentum, `buf` is never touched; 1: momentum; 2: Nesterov momentum.
template <int MOM, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_sgd(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, int64_t n4,
                                              const SgdGroupTable tab, float momentum, float gscale, const uint8_t* __restrict__ ids,
                                              float max_norm, const double* __restrict__ partial, int npartial, float* __restrict__ ema,
                                              float ema_decay, uint32_t* __restrict__ status) {
    float coef = 1.f;
    if (CLIP) {
        __shared__ double red[4];
        bool finite;
        coef = clip_coef_256(partial, npartial, gscale, max_norm, red, status, blockIdx.x == 0 && threadIdx.x == 0, finite);
        if (!finite) return;                                                   // skipped for every group: nothing is written
    }
    const uint32_t lane = threadIdx.x & 63u, row = lane & (SD_OPTIM_MAX_GROUPS - 1u);
    float row_lr = tab.lr[0], row_wd = tab.wd[0];
#pragma unroll
    for (uint32_t q = 1; q < SD_OPTIM_MAX_GROUPS; ++q) {
        row_lr = row == q ? tab.lr[q] : row_lr;
        row_wd = row == q ? tab.wd[q] : row_wd;
    }
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x - lane); base < n4; base += stride) {     // per wave, as in k_optim_groups
        const int64_t i = base + lane;
        const bool live = i < n4;
        const uint32_t k = live ? ids[i] & (SD_OPTIM_MAX_GROUPS - 1u) : 0u;
        const float lr = __shfl(row_lr, (int)k), wd = __shfl(row_wd, (int)k);
        if (!live) continue;
        float4 pp = reinterpret_cast<float4*>(p)[i];
        const float4 gg = reinterpret_cast<const float4*>(g)[i];
        float4 bb = make_float4(0.f, 0.f, 0.f, 0.f), ee = make_float4(0.f, 0.f, 0.f, 0.f);
        if (MOM) bb = reinterpret_cast<float4*>(buf)[i];
        if (EMA) ee = reinterpret_cast<float4*>(ema)[i];
        float* P = &pp.x; const float* G = &gg.x; float* Bu = &bb.x; float* E = &ee.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float d = G[j] * gscale;
            if (CLIP) d *= coef;
            if (wd > 0.f) d += wd * P[j];                            // coupled L2: grad.add(param, alpha=weight_decay)
            if (MOM) {
                Bu[j] = momentum * Bu[j] + d;                        // buf.mul_(momentum).add_(grad); a zero buffer at step 1: buf = grad
                d = MOM == 2 ? d + momentum * Bu[j] : Bu[j];
            }
            P[j] -= lr * d;
            if (EMA) E[j] = ema_decay * E[j] + (1.f - ema_decay) * P[j];
        }
        reinterpret_cast<float4*>(p)[i] = pp;
        if (MOM) reinterpret_cast<float4*>(buf)[i] = bb;
        if (EMA) reinterpret_cast<float4*>(ema)[i] = ee;
    }
}

// LAMB.  The slot table (sd_lamb_table_build; int32, on the device): [nslots] rows {lo4, hi4, first block, block count | adapt << 30} in
// float4 units, then [nblocks] slot indices, one per block.  A block works on ONE slot: block b of a slot's nb blocks takes the float4s
// lo4 + (r * nb + b) * 1024 + [0, 1024) for r = 0, 1, .. (one "sweep" of the slot per r), a thread its four of each 1024 in index order.
// Every value read from the table is clamped before it is used as an index: a wrong table gives wrong numbers inside [0, n4) and
// inside the workspace, never an access outside them.
constexpr int LAMB_BLOCK_F4 = SD_LAMB_BLOCK_FLOATS / 4;
static_assert(LAMB_BLOCK_F4 == 4 * 256 && SD_LAMB_MAX_SLOT_BLOCKS <= 256, "k_lamb_*: four float4 a thread and a sweep, a slot's partials in one read a thread");

struct LambSlot { int64_t lo4, hi4; int first, nb, bi; bool adapt; };

__device__ __forceinline__ LambSlot lamb_slot(const int32_t* __restrict__ table, int nslots, int nblocks, int64_t n4) {
    const int s = min(max(table[4 * (int64_t)nslots + blockIdx.x], 0), nslots - 1);
    const int4 e = reinterpret_cast<const int4*>(table)[s];
    LambSlot o;
    o.lo4 = min((int64_t)max(e.x, 0), n4);
    o.hi4 = min(max((int64_t)e.y, o.lo4), n4);
    o.first = min(max(e.z, 0), nblocks - 1);
    o.nb = min(min(max(e.w & 0xffff, 1), SD_LAMB_MAX_SLOT_BLOCKS), nblocks - o.first);
    o.bi = min(max((int)blockIdx.x - o.first, 0), o.nb - 1);
    o.adapt = (e.w >> 30 & 1) != 0;
    return o;
}

// u of one element from the moments as they are stored; no multiply-add is left to contraction, so that both passes get the same bits
__device__ __forceinline__ float lamb_u(float m, float v, float p, float bc1, float bc2_sqrt, float eps, float wd) {
    const float u = (m / bc1) / (sqrtf(v) / bc2_sqrt + eps);
    return wd > 0.f ? __builtin_fmaf(wd, p, u) : u;
}

// pass 1: the moments, and this block's fp64 (sum p^2, sum u^2) into workspace[2 * block], [2 * block + 1]
template <bool CLIP>
__global__ __launch_bounds__(256) void k_lamb_moments(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, int64_t n4, const SgdGroupTable tab, float b1, float b2, float eps,
                                                       float bc1, float bc2_sqrt, float gscale, const uint8_t* __restrict__ ids, float max_norm,
                                                       const double* __restrict__ partial, int npartial, uint32_t* __restrict__ status,
                                                       const int32_t* __restrict__ table, int nslots, int nblocks, double* __restrict__ ws) {
    __shared__ double red[4], red_p[4], red_u[4];
    __shared__ float s_wd[SD_OPTIM_MAX_GROUPS];
    float coef = 1.f;
    if (CLIP) {
        bool finite;
        coef = clip_coef_256(partial, npartial, gscale, max_norm, red, status, blockIdx.x == 0 && threadIdx.x == 0, finite);
        if (!finite) return;
    }
    if (threadIdx.x < SD_OPTIM_MAX_GROUPS) s_wd[threadIdx.x] = tab.wd[threadIdx.x];
    __syncthreads();
    const LambSlot sl = lamb_slot(table, nslots, nblocks, n4);
    double sp = 0.0, su = 0.0;
    for (int64_t base = sl.lo4 + (int64_t)sl.bi * LAMB_BLOCK_F4; base < sl.hi4; base += (int64_t)sl.nb * LAMB_BLOCK_F4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = base + q * 256 + threadIdx.x;
            if (i >= sl.hi4) continue;
            const float4 pp = reinterpret_cast<const float4*>(p)[i], gg = reinterpret_cast<const float4*>(g)[i];
            float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
            const float wd = s_wd[ids[i] & (SD_OPTIM_MAX_GROUPS - 1u)];
            const float* P = &pp.x; const float* G = &gg.x; float* Mo = &mm.x; float* V = &vv.x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float gr = G[j] * gscale;
                if (CLIP) gr *= coef;
                Mo[j] = b1 * Mo[j] + (1.f - b1) * gr;
                V[j] = b2 * V[j] + (1.f - b2) * gr * gr;
                const float u = lamb_u(Mo[j], V[j], P[j], bc1, bc2_sqrt, eps, wd);
                sp += (double)P[j] * P[j];
                su += (double)u * u;
            }
            reinterpret_cast<float4*>(m)[i] = mm;
            reinterpret_cast<float4*>(v)[i] = vv;
        }
    }
    sp = block_sum_256(sp, red_p);
    su = block_sum_256(su, red_u);
    if (threadIdx.x == 0) {
        ws[2 * (int64_t)blockIdx.x] = sp;
        ws[2 * (int64_t)blockIdx.x + 1] = su;
    }
}

// pass 2: every block finishes its slot's partials itself (at most SD_LAMB_MAX_SLOT_BLOCKS pairs, in block order), recomputes u from the
// stored moments and the parameter it is about to change, and applies p -= lr_k * phi * u
template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_lamb_apply(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v, int64_t n4,
                                                     const SgdGroupTable tab, float eps, float bc1, float bc2_sqrt, float gscale,
                                                     const uint8_t* __restrict__ ids, float max_norm, const double* __restrict__ partial,
                                                     int npartial, float* __restrict__ ema, float ema_decay, const int32_t* __restrict__ table,
                                                     int nslots, int nblocks, const double* __restrict__ ws) {
    __shared__ double red[4], red_p[4], red_u[4];
    __shared__ float s_lr[SD_OPTIM_MAX_GROUPS], s_wd[SD_OPTIM_MAX_GROUPS];
    if (CLIP) {
        bool finite;
        clip_coef_256(partial, npartial, gscale, max_norm, red, nullptr, false, finite);   // pass 1 recorded the status; the same partials, the same verdict
        if (!finite) return;
    }
    if (threadIdx.x < SD_OPTIM_MAX_GROUPS) {
        s_lr[threadIdx.x] = tab.lr[threadIdx.x];
        s_wd[threadIdx.x] = tab.wd[threadIdx.x];
    }
    const LambSlot sl = lamb_slot(table, nslots, nblocks, n4);
    double sp = 0.0, su = 0.0;
    for (int k = threadIdx.x; k < sl.nb; k += 256) {
        sp += ws[2 * (int64_t)(sl.first + k)];
        su += ws[2 * (int64_t)(sl.first + k) + 1];
    }
    sp = block_sum_256(sp, red_p);                                             // (its barrier also publishes s_lr / s_wd)
    su = block_sum_256(su, red_u);
    const double norm_p = sqrt(sp), norm_u = sqrt(su);
    const bool trust = sl.adapt && norm_p > 0.0 && norm_u > 0.0 && norm_p < HUGE_VAL && norm_u < HUGE_VAL;   // (false for nan)
    const float phi = trust ? (float)(norm_p / norm_u) : 1.f;
    for (int64_t base = sl.lo4 + (int64_t)sl.bi * LAMB_BLOCK_F4; base < sl.hi4; base += (int64_t)sl.nb * LAMB_BLOCK_F4) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = base + q * 256 + threadIdx.x;
            if (i >= sl.hi4) continue;
            float4 pp = reinterpret_cast<float4*>(p)[i];
            const float4 mm = reinterpret_cast<const float4*>(m)[i], vv = reinterpret_cast<const float4*>(v)[i];
            float4 ee = make_float4(0.f, 0.f, 0.f, 0.f);
            if (EMA) ee = reinterpret_cast<float4*>(ema)[i];
            const uint32_t k = ids[i] & (SD_OPTIM_MAX_GROUPS - 1u);
            const float step = s_lr[k] * phi, wd = s_wd[k];
            float* P = &pp.x; const float* Mo = &mm.x; const float* V = &vv.x; float* E = &ee.x;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                P[j] -= step * lamb_u(Mo[j], V[j], P[j], bc1, bc2_sqrt, eps, wd);
                if (EMA) E[j] = ema_decay * E[j] + (1.f - ema_decay) * P[j];
            }
            reinterpret_cast<float4*>(p)[i] = pp;
            if (EMA) reinterpret_cast<float4*>(ema)[i] = ee;
        }
    }
}

// Gradient accumulation (sd_grad_accum): dst += src, or dst = src for the first micro-batch of a group (no zero-fill pass before it).
// One fp32 add per element, written as four separate adds so that nothing can contract them; a streaming pass of 12 (8) bytes per float.
// dst and src may be the SAME range (the entry point refuses any other overlap), so neither pointer is __restrict__.
template <bool OVERWRITE>
__global__ __launch_bounds__(256) void k_grad_accum(float* dst, const float* src, int64_t n4) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 s = reinterpret_cast<const float4*>(src)[i];
        if (!OVERWRITE) {
            const float4 d = reinterpret_cast<const float4*>(dst)[i];
            s.x = d.x + s.x; s.y = d.y + s.y; s.z = d.z + s.z; s.w = d.w + s.w;
        }
        reinterpret_cast<float4*>(dst)[i] = s;
    }
}

// ------------------------------------------------------------------------------------------
// bf16 backbone (inference): weight cast, max-pool and head reading bf16 NHWC activations
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float bf2f_(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ uint16_t f2bf_(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }

__global__ __launch_bounds__(256) void k_cast_bf16(const float* __restrict__ x, uint16_t* __restrict__ y, int64_t n4) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        reinterpret_cast<ushort4*>(y)[i] = make_ushort4(f2bf_(v.x), f2bf_(v.y), f2bf_(v.z), f2bf_(v.w));
    }
}

__global__ __launch_bounds__(256) void k_cast_f32(const uint16_t* __restrict__ x, float* __restrict__ y, int64_t n4) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) st4(y, i, ld4(x, i));
}

__global__ __launch_bounds__(256) void k_maxpool_fwd_bf16(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int B, int Hi, int Wi,
                                                           int Ho, int Wo, int C) {
    const int cols = C >> 3;                       // 8 bf16 = 16 bytes per thread
    const int64_t n8 = (int64_t)B * Ho * Wo * cols;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int col = (int)(i % cols);
    int64_t t = i / cols;
    const int ox = (int)(t % Wo); t /= Wo;
    const int oy = (int)(t % Ho);
    const int b = (int)(t / Ho);
    float m[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = -INFINITY;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            const int iy = oy * 2 - 1 + r, ix = ox * 2 - 1 + s;
            if (iy < 0 || iy >= Hi || ix < 0 || ix >= Wi) continue;
            const uint4 v = reinterpret_cast<const uint4*>(x + (((int64_t)b * Hi + iy) * Wi + ix) * C)[col];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                m[2 * j] = fmaxf(m[2 * j], __uint_as_float(w[j] << 16));
                m[2 * j + 1] = fmaxf(m[2 * j + 1], __uint_as_float(w[j] & 0xffff0000u));
            }
        }
    uint4 o;
    o.x = (uint32_t)f2bf_(m[0]) | ((uint32_t)f2bf_(m[1]) << 16); o.y = (uint32_t)f2bf_(m[2]) | ((uint32_t)f2bf_(m[3]) << 16);
    o.z = (uint32_t)f2bf_(m[4]) | ((uint32_t)f2bf_(m[5]) << 16); o.w = (uint32_t)f2bf_(m[6]) | ((uint32_t)f2bf_(m[7]) << 16);
    reinterpret_cast<uint4*>(y)[i] = o;
}

// head on a bf16 NHWC input: fp32 weights / accumulation / NCHW output (the decoder always runs in fp32)
__global__ __launch_bounds__(256) void k_head_fwd_bf16(const uint16_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int64_t M, int HW, int C, int Co) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int LD = C + 4;
    float* xs = lds;                 // [64][C+4] fp32
    float* ws = lds + 64 * LD;       // [Co][C]
    const int64_t m0 = (int64_t)blockIdx.x * 64;
    const int c8 = C >> 3;
    for (int i = threadIdx.x; i < 64 * c8; i += 256) {
        const int row = i / c8, col = i - row * c8;
        const int64_t m = m0 + row;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (m < M) v = reinterpret_cast<const uint4*>(x + m * C)[col];
        float* d = xs + row * LD + col * 8;
        d[0] = __uint_as_float(v.x << 16); d[1] = __uint_as_float(v.x & 0xffff0000u);
        d[2] = __uint_as_float(v.y << 16); d[3] = __uint_as_float(v.y & 0xffff0000u);
        d[4] = __uint_as_float(v.z << 16); d[5] = __uint_as_float(v.z & 0xffff0000u);
        d[6] = __uint_as_float(v.w << 16); d[7] = __uint_as_float(v.w & 0xffff0000u);
    }
    for (int i = threadIdx.x; i < Co * C; i += 256) ws[i] = w[i];
    __syncthreads();
    const int px = threadIdx.x & 63, grp = threadIdx.x >> 6;
    float acc[HEAD_NARROW_MAX_CO / 4];
#pragma unroll
    for (int j = 0; j < HEAD_NARROW_MAX_CO / 4; ++j) acc[j] = 0.f;
    for (int c = 0; c < C; c += 4) {
        const float4 v = *reinterpret_cast<const float4*>(xs + px * LD + c);
#pragma unroll
        for (int j = 0; j < HEAD_NARROW_MAX_CO / 4; ++j) {
            const int co = grp + 4 * j;
            if (co < Co) {
                const float4 ww = *reinterpret_cast<const float4*>(ws + co * C + c);
                acc[j] += v.x * ww.x + v.y * ww.y + v.z * ww.z + v.w * ww.w;
            }
        }
    }
    const int64_t m = m0 + px;
    if (m < M) {
        const int64_t b = m / HW, pix = m - b * HW;
#pragma unroll
        for (int j = 0; j < HEAD_NARROW_MAX_CO / 4; ++j) {
            const int co = grp + 4 * j;
            if (co < Co) y[(b * Co + co) * HW + pix] = acc[j] + bias[co];
        }
    }
}

// Head on a bf16 NHWC input of 128 channels (the default FPN depth), wave-private pipeline: every wave walks tiles of 64 pixels; the
// tile (16 KB) comes in by LDS-DMA (16 wave-instructions of 1 KB, no staging registers, no block barrier) and is multiplied on the
// bf16 MFMA with the fp32 weights split into two bf16 terms, w = hi + lo (|w - hi - lo| <= 2^-17 |w|: the activations are bf16
// already, so x * hi + x * lo summed in fp32 equals the fp32 product to fp32 rounding).  Co <= 16: hi sits in columns 0 .. 15 and lo
// in columns 16 .. 31 of ONE 32-column B operand (the two halves are added across lanes at the end); Co <= 32: two MFMAs per step.
// The Co planes of the NCHW output are written 16 bytes (4 pixels) per lane.  k_head_fwd_bf16 staged 64 pixels per BLOCK, widened to
// fp32, and re-read every row once per output-channel group (24x the input bytes in LDS traffic): 186 us for 268 MB at bs=64.
//   LDS image of a tile: row r (pixel) x 16 slots of 16 bytes, slot c of row r at physical slot c ^ (r & 15): the DMA lane that lands in
//   physical slot s of row r fetches chunk s ^ (r & 15) (swizzle on the SOURCE), and the 16 lanes of a ds_read_b128 group (rows r ..
//   r+15, same chunk) hit 16 different slots.
typedef float head_f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 head_bf16x8 __attribute__((ext_vector_type(8)));
template <bool SPLIT>
__global__ __launch_bounds__(256) void k_head_fwd_bf16_c128(const uint16_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                             float* __restrict__ y, int64_t M, int HW, int Co, int ntiles) {
    __shared__ __attribute__((aligned(16))) float lds[4 * 4096];              // 16 KB per wave
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* T = lds + wave * 4096;
    const int nwaves = gridDim.x * 4;
    const int rsub = lane >> 4, slot = lane & 15;                              // DMA: lane -> (row within a 4-row piece, physical slot)
    const int fr = lane & 31, fh = lane >> 5;
    // B operands: lane (n = fr, k-half fh) holds w[n][16 s + 8 fh .. + 7] of step s as bf16
    head_bf16x8 bh[8], bl[8];
    {
        const int n = SPLIT ? fr : (fr & 15);
        const bool lo_col = !SPLIT && fr >= 16;
#pragma unroll
        for (int st = 0; st < 8; ++st) {
            uint16_t h[8], l[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const float wv = n < Co ? w[n * 128 + 16 * st + 8 * fh + k] : 0.f;
                const uint16_t hi = f32_to_bf16(wv);
                const uint16_t lo = f32_to_bf16(wv - bf16_to_f32(hi));
                h[k] = lo_col ? lo : hi; l[k] = lo;
            }
            bh[st] = __builtin_bit_cast(head_bf16x8, h);
            bl[st] = __builtin_bit_cast(head_bf16x8, l);
        }
    }
    const float bv = (fr < Co && (SPLIT || fr < 16)) ? bias[fr] : 0.f;
    for (int tile = blockIdx.x * 4 + wave; tile < ntiles; tile += nwaves) {
        const int64_t m0 = (int64_t)tile * 64;
#pragma unroll
        for (int pc = 0; pc < 16; ++pc) {
            const int r = pc * 4 + rsub;
            const int64_t m = min(m0 + r, M - 1);                              // (rows past the end re-read the last pixel; never stored)
#if defined(__HIP_DEVICE_COMPILE__)
            const uint16_t* src = x + m * 128 + ((slot ^ (r & 15)) << 3);
            __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(T + pc * 256), 16, 0, 0);
#else
            (void)m; (void)slot;
#endif
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        head_f32x16 acc[2], accl[2];
#pragma unroll
        for (int mi = 0; mi < 2; ++mi)
#pragma unroll
            for (int e = 0; e < 16; ++e) { acc[mi][e] = 0.f; accl[mi][e] = 0.f; }
#pragma unroll
        for (int st = 0; st < 8; ++st) {
#pragma unroll
            for (int mi = 0; mi < 2; ++mi) {
                const int r = mi * 32 + fr;
                const head_bf16x8 a = *reinterpret_cast<const head_bf16x8*>(reinterpret_cast<const char*>(T) + r * 256 + (((2 * st + fh) ^ (r & 15)) << 4));
                acc[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bh[st], acc[mi], 0, 0, 0);
                if (SPLIT) accl[mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, bl[st], accl[mi], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     // every LDS read of this tile is done before the next tile's DMA lands
        // C/D map of the 32x32 MFMA: column (output channel) = lane & 31, rows (pixels) (e & 3) + 8 (e >> 2) + 4 fh: four consecutive pixels per e >> 2
#pragma unroll
        for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 o;
                float* op = &o.x;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float hi = acc[mi][4 * g + k];
                    const float lo = SPLIT ? accl[mi][4 * g + k] : __shfl_down(hi, 16);      // column n + 16 holds x * lo
                    op[k] = hi + lo + bv;
                }
                const int64_t m = m0 + mi * 32 + 8 * g + 4 * fh;
                if (fr < Co && (SPLIT || fr < 16) && m < M) {
                    const int64_t b = m / HW, pix = m - b * HW;                // (HW % 4 == 0: the four pixels stay in one image)
                    *reinterpret_cast<float4*>(y + (b * Co + fr) * HW + pix) = o;
                }
            }
        }
    }
}

// ---- bf16 activations, 16 bytes per lane (8 elements): the mixed-precision training path's BatchNorm passes.  Same arithmetic
// as the templated 4-element kernels above (fp32, one rounding at the store; results are bit-identical to them) -- only the
// access width differs: 8-byte accesses left these HBM-bound passes at ~60 % of the rate of their fp32 (16-byte) versions.
struct F8 { float4 a, b; };
__device__ __forceinline__ F8 ld8(const uint16_t* p, int64_t i) {
    typedef unsigned sd_u32x4_nt __attribute__((ext_vector_type(4)));               // (read once: non-temporal, see ld4 in sd_common.h)
    const sd_u32x4_nt r_ = __builtin_nontemporal_load(reinterpret_cast<const sd_u32x4_nt*>(p) + i);
    const uint4 r = make_uint4(r_[0], r_[1], r_[2], r_[3]);
    F8 v;
    v.a = make_float4(bf16_to_f32((uint16_t)(r.x & 0xffff)), bf16_to_f32((uint16_t)(r.x >> 16)), bf16_to_f32((uint16_t)(r.y & 0xffff)), bf16_to_f32((uint16_t)(r.y >> 16)));
    v.b = make_float4(bf16_to_f32((uint16_t)(r.z & 0xffff)), bf16_to_f32((uint16_t)(r.z >> 16)), bf16_to_f32((uint16_t)(r.w & 0xffff)), bf16_to_f32((uint16_t)(r.w >> 16)));
    return v;
}
__device__ __forceinline__ void st8(uint16_t* p, int64_t i, const F8& v) {
    uint4 r;
    r.x = (uint32_t)f32_to_bf16(v.a.x) | ((uint32_t)f32_to_bf16(v.a.y) << 16); r.y = (uint32_t)f32_to_bf16(v.a.z) | ((uint32_t)f32_to_bf16(v.a.w) << 16);
    r.z = (uint32_t)f32_to_bf16(v.b.x) | ((uint32_t)f32_to_bf16(v.b.y) << 16); r.w = (uint32_t)f32_to_bf16(v.b.z) | ((uint32_t)f32_to_bf16(v.b.w) << 16);
    reinterpret_cast<uint4*>(p)[i] = r;
}

__global__ __launch_bounds__(256) void k_bn_apply_bf16x8(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int64_t n8, int C,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          const uint16_t* __restrict__ res, int relu, uint8_t* __restrict__ mask) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int cols = C >> 3;
    const bool fixed = stride % cols == 0;                      // (see k_bn_apply: one column per thread; here EIGHT parameter vectors per element)
    const int col0 = (int)(((int64_t)blockIdx.x * 256 + threadIdx.x) % cols);
    float4 mu[2], is[2], g[2], b[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        mu[h] = reinterpret_cast<const float4*>(mean)[2 * col0 + h]; is[h] = reinterpret_cast<const float4*>(invstd)[2 * col0 + h];
        g[h] = reinterpret_cast<const float4*>(gamma)[2 * col0 + h]; b[h] = reinterpret_cast<const float4*>(beta)[2 * col0 + h];
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const F8 v = ld8(x, i);
        if (!fixed) {
            const int col = (int)(i % cols);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                mu[h] = reinterpret_cast<const float4*>(mean)[2 * col + h]; is[h] = reinterpret_cast<const float4*>(invstd)[2 * col + h];
                g[h] = reinterpret_cast<const float4*>(gamma)[2 * col + h]; b[h] = reinterpret_cast<const float4*>(beta)[2 * col + h];
            }
        }
        F8 o;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 vv = h ? v.b : v.a;
            float4 oo;
            oo.x = (vv.x - mu[h].x) * is[h].x * g[h].x + b[h].x; oo.y = (vv.y - mu[h].y) * is[h].y * g[h].y + b[h].y;
            oo.z = (vv.z - mu[h].z) * is[h].z * g[h].z + b[h].z; oo.w = (vv.w - mu[h].w) * is[h].w * g[h].w + b[h].w;
            if (h) o.b = oo; else o.a = oo;
        }
        if (res) {
            const F8 r = ld8(res, i);
            o.a.x += r.a.x; o.a.y += r.a.y; o.a.z += r.a.z; o.a.w += r.a.w; o.b.x += r.b.x; o.b.y += r.b.y; o.b.z += r.b.z; o.b.w += r.b.w;
        }
        if (mask) {        // one byte per FOUR elements, as the 4-element kernels write it
            const uint8_t m0 = (uint8_t)((o.a.x > 0.f ? 1 : 0) | (o.a.y > 0.f ? 2 : 0) | (o.a.z > 0.f ? 4 : 0) | (o.a.w > 0.f ? 8 : 0));
            const uint8_t m1 = (uint8_t)((o.b.x > 0.f ? 1 : 0) | (o.b.y > 0.f ? 2 : 0) | (o.b.z > 0.f ? 4 : 0) | (o.b.w > 0.f ? 8 : 0));
            reinterpret_cast<uchar2*>(mask)[i] = make_uchar2(m0, m1);
        }
        if (relu) {
            o.a.x = fmaxf(o.a.x, 0.f); o.a.y = fmaxf(o.a.y, 0.f); o.a.z = fmaxf(o.a.z, 0.f); o.a.w = fmaxf(o.a.w, 0.f);
            o.b.x = fmaxf(o.b.x, 0.f); o.b.y = fmaxf(o.b.y, 0.f); o.b.z = fmaxf(o.b.z, 0.f); o.b.w = fmaxf(o.b.w, 0.f);
        }
        st8(y, i, o);
    }
}

// g = dy * relu mask (relu: 0 none, 2 recomputed from x, 3 mask bytes) for one float4 half
__device__ __forceinline__ float4 bn_mask4(float4 g, const float4 xv, const float4 mu, const float4 is, const float4 ga, const float4 be, int relu, uint8_t mb) {
    if (relu == 3) {
        g.x = (mb & 1) ? g.x : 0.f; g.y = (mb & 2) ? g.y : 0.f; g.z = (mb & 4) ? g.z : 0.f; g.w = (mb & 8) ? g.w : 0.f;
    } else if (relu == 2) {
        g.x = ((xv.x - mu.x) * is.x * ga.x + be.x) > 0.f ? g.x : 0.f; g.y = ((xv.y - mu.y) * is.y * ga.y + be.y) > 0.f ? g.y : 0.f;
        g.z = ((xv.z - mu.z) * is.z * ga.z + be.z) > 0.f ? g.z : 0.f; g.w = ((xv.w - mu.w) * is.w * ga.w + be.w) > 0.f ? g.w : 0.f;
    }
    return g;
}

__global__ __launch_bounds__(256) void k_bn_bwd_apply_bf16x8(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ x, const uint8_t* __restrict__ maskb,
                                                              int relu, int64_t n8, int C, const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const float* __restrict__ mg,
                                                              const float* __restrict__ mgx, uint16_t* __restrict__ dx, uint16_t* __restrict__ g_out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int cols = C >> 3;
    const bool fixed = stride % cols == 0;                      // (see k_bn_apply: one column per thread; here up to TWELVE parameter vectors per element)
    const int col0 = (int)(((int64_t)blockIdx.x * 256 + threadIdx.x) % cols);
    float4 mu[2], is[2], ga[2], be[2], a[2], b[2];
    auto params = [&](int col) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            mu[h] = reinterpret_cast<const float4*>(mean)[2 * col + h]; is[h] = reinterpret_cast<const float4*>(invstd)[2 * col + h];
            ga[h] = reinterpret_cast<const float4*>(gamma)[2 * col + h];
            be[h] = relu == 2 ? reinterpret_cast<const float4*>(beta)[2 * col + h] : make_float4(0.f, 0.f, 0.f, 0.f);
            a[h] = reinterpret_cast<const float4*>(mg)[2 * col + h]; b[h] = reinterpret_cast<const float4*>(mgx)[2 * col + h];
        }
    };
    params(col0);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += stride) {
        const F8 gy = ld8(dy, i), xv = ld8(x, i);
        if (!fixed) params((int)(i % cols));
        uchar2 mb = make_uchar2(0, 0);
        if (relu == 3) mb = reinterpret_cast<const uchar2*>(maskb)[i];
        F8 o, gm;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const float4 xx = h ? xv.b : xv.a;
            const float4 g = bn_mask4(h ? gy.b : gy.a, xx, mu[h], is[h], ga[h], be[h], relu, h ? mb.y : mb.x);
            float4 oo;
            oo.x = ga[h].x * is[h].x * (g.x - a[h].x - (xx.x - mu[h].x) * is[h].x * b[h].x);
            oo.y = ga[h].y * is[h].y * (g.y - a[h].y - (xx.y - mu[h].y) * is[h].y * b[h].y);
            oo.z = ga[h].z * is[h].z * (g.z - a[h].z - (xx.z - mu[h].z) * is[h].z * b[h].z);
            oo.w = ga[h].w * is[h].w * (g.w - a[h].w - (xx.w - mu[h].w) * is[h].w * b[h].w);
            if (h) { o.b = oo; gm.b = g; } else { o.a = oo; gm.a = g; }
        }
        st8(dx, i, o);
        if (g_out) st8(g_out, i, gm);
    }
}

// BatchNorm-backward reduction (k_col_reduce<1>) on bf16, 8 columns per lane: sum g, sum g * xhat per channel
__global__ __launch_bounds__(256) void k_col_reduce_bwd_bf16x8(const uint16_t* __restrict__ a, const uint16_t* __restrict__ b, const uint8_t* __restrict__ maskb,
                                                                const float* __restrict__ mean, const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma, const float* __restrict__ beta, int relu,
                                                                int64_t M, int C, float* __restrict__ partial, int rpb) {
    __shared__ float4 red[4][256];
    const int cols = C >> 3;                       // 8-element columns (cols <= 128 for C <= 1024)
    const int lanes = 256 / cols;
    const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(r0 + rpb, M);
    float4 s0[2], s1[2], mu[2], is[2], ga[2], be[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        s0[h] = s1[h] = ga[h] = be[h] = make_float4(0.f, 0.f, 0.f, 0.f);
        mu[h] = reinterpret_cast<const float4*>(mean)[2 * col + h]; is[h] = reinterpret_cast<const float4*>(invstd)[2 * col + h];
        if (relu == 2) { ga[h] = reinterpret_cast<const float4*>(gamma)[2 * col + h]; be[h] = reinterpret_cast<const float4*>(beta)[2 * col + h]; }
    }
    if (rl < lanes) {
#pragma unroll 2
        for (int64_t r = r0 + rl; r < r1; r += lanes) {
            const F8 gy = ld8(a, r * cols + col), xv = ld8(b, r * cols + col);
            uchar2 mb = make_uchar2(0, 0);
            if (relu == 3) mb = reinterpret_cast<const uchar2*>(maskb)[r * cols + col];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 xx = h ? xv.b : xv.a;
                const float4 g = bn_mask4(h ? gy.b : gy.a, xx, mu[h], is[h], ga[h], be[h], relu, h ? mb.y : mb.x);
                s0[h].x += g.x; s0[h].y += g.y; s0[h].z += g.z; s0[h].w += g.w;
                s1[h].x += g.x * ((xx.x - mu[h].x) * is[h].x); s1[h].y += g.y * ((xx.y - mu[h].y) * is[h].y);
                s1[h].z += g.z * ((xx.z - mu[h].z) * is[h].z); s1[h].w += g.w * ((xx.w - mu[h].w) * is[h].w);
            }
        }
    }
    red[0][threadIdx.x] = s0[0]; red[1][threadIdx.x] = s0[1]; red[2][threadIdx.x] = s1[0]; red[3][threadIdx.x] = s1[1];
    __syncthreads();
    if (rl == 0) {
        for (int l = 1; l < lanes; ++l) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 u = red[h][l * cols + col], w = red[2 + h][l * cols + col];
                s0[h].x += u.x; s0[h].y += u.y; s0[h].z += u.z; s0[h].w += u.w;
                s1[h].x += w.x; s1[h].y += w.y; s1[h].z += w.z; s1[h].w += w.w;
            }
        }
        float* dst = partial + (int64_t)blockIdx.x * 2 * C;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            reinterpret_cast<float4*>(dst)[2 * col + h] = s0[h];
            reinterpret_cast<float4*>(dst + C)[2 * col + h] = s1[h];
        }
    }
}

// ---- frozen BatchNorm, backward (sd_frozen_bn_bwd): g = dy * [y > 0] (y null: no ReLU), dx = g * scale[c], optionally g_out = g.  The layer
// is the per-channel affine of sd_bn_fold, so there is nothing to reduce: one streaming pass, dy (and y) in, dx (and g) out.  The vector
// kernels take a float4 / 8 bf16 per thread and step: the grid stride is a multiple of 256 and the column count (C/4, C/8) divides 256, so a
// thread never leaves its column and keeps its scales in registers.  The element-wise kernel (a misaligned pointer, bf16 with C % 8 != 0)
// stages the scales in LDS.
__global__ __launch_bounds__(256) void k_bn_frozen_bwd_f32x4(const float* __restrict__ dy, const float* __restrict__ y, const float* __restrict__ scale,
                                                              int64_t n4, int C, float* __restrict__ dx, float* __restrict__ g_out) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c0 = 4 * (int)(i0 % (C >> 2));
    const float s0 = scale[c0], s1 = scale[c0 + 1], s2 = scale[c0 + 2], s3 = scale[c0 + 3];
    for (int64_t i = i0; i < n4; i += stride) {
        float4 g = ld4(dy, i);
        if (y) {
            const float4 yy = ld4(y, i);
            g.x = yy.x > 0.f ? g.x : 0.f; g.y = yy.y > 0.f ? g.y : 0.f; g.z = yy.z > 0.f ? g.z : 0.f; g.w = yy.w > 0.f ? g.w : 0.f;
        }
        st4(dx, i, make_float4(g.x * s0, g.y * s1, g.z * s2, g.w * s3));
        if (g_out) st4(g_out, i, g);
    }
}

// two bf16 of a dword: the gradient where the ReLU output is positive (its own bits), +0 elsewhere / times their scales, rounded to nearest even
__device__ __forceinline__ uint32_t frozen_mask2(uint32_t d, uint32_t y) {
    return (bf16_to_f32((uint16_t)(y & 0xffffu)) > 0.f ? (d & 0xffffu) : 0u) | (bf16_to_f32((uint16_t)(y >> 16)) > 0.f ? (d & 0xffff0000u) : 0u);
}
__device__ __forceinline__ uint32_t frozen_scale2(uint32_t g, float s0, float s1) {
    return (uint32_t)f32_to_bf16(bf16_to_f32((uint16_t)(g & 0xffffu)) * s0) | ((uint32_t)f32_to_bf16(bf16_to_f32((uint16_t)(g >> 16)) * s1) << 16);
}

__global__ __launch_bounds__(256) void k_bn_frozen_bwd_bf16x8(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ y, const float* __restrict__ scale,
                                                               int64_t n8, int C, uint16_t* __restrict__ dx, uint16_t* __restrict__ g_out) {
    typedef unsigned sd_u32x4_nt __attribute__((ext_vector_type(4)));               // (read once: non-temporal, see ld4 in sd_common.h)
    const int64_t stride = (int64_t)gridDim.x * 256;
    const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c0 = 8 * (int)(i0 % (C >> 3));
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = scale[c0 + j];
    for (int64_t i = i0; i < n8; i += stride) {
        const sd_u32x4_nt d = __builtin_nontemporal_load(reinterpret_cast<const sd_u32x4_nt*>(dy) + i);
        uint4 g = make_uint4(d[0], d[1], d[2], d[3]);
        if (y) {
            const sd_u32x4_nt m = __builtin_nontemporal_load(reinterpret_cast<const sd_u32x4_nt*>(y) + i);
            g = make_uint4(frozen_mask2(g.x, m[0]), frozen_mask2(g.y, m[1]), frozen_mask2(g.z, m[2]), frozen_mask2(g.w, m[3]));
        }
        reinterpret_cast<uint4*>(dx)[i] = make_uint4(frozen_scale2(g.x, s[0], s[1]), frozen_scale2(g.y, s[2], s[3]), frozen_scale2(g.z, s[4], s[5]),
                                                     frozen_scale2(g.w, s[6], s[7]));
        if (g_out) reinterpret_cast<uint4*>(g_out)[i] = g;
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_bn_frozen_bwd_ew(const T* __restrict__ dy, const T* __restrict__ y, const float* __restrict__ scale, int64_t n,
                                                           int C, T* __restrict__ dx, T* __restrict__ g_out) {
    __shared__ float s[1024];                                                       // C <= 1024 (check_mc)
    for (int c = threadIdx.x; c < C; c += 256) s[c] = scale[c];
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float sc = s[(int)(i % C)];
        if constexpr (std::is_same<T, float>::value) {
            const float g = (!y || y[i] > 0.f) ? dy[i] : 0.f;
            dx[i] = g * sc;
            if (g_out) g_out[i] = g;
        } else {
            const uint16_t g = (!y || bf16_to_f32(y[i]) > 0.f) ? dy[i] : (uint16_t)0;
            dx[i] = f32_to_bf16(bf16_to_f32(g) * sc);
            if (g_out) g_out[i] = g;
        }
    }
}

static inline int ew_grid(int64_t n4) { return (int)std::min<int64_t>(cdiv(n4, 256), 256 * 16); }

}  // namespace sd
#include <cstdarg>                                    // (va_list: the formatter of sd_nn_kernel_names)

using namespace sd;

// ==== host layer: checks (one checker per argument family, the entry point's name passed as `what`), a plan (plain structs, no HIP call, no
// allocation), the launches the plan names.  sd_nn_kernel_names at the end prints the same plans; nothing else here formats a string. =========

static thread_local int g_pool_pair = 1;              // sd_set_option("pool_fwd_pair", 0): one window per thread in sd_bn_relu_maxpool_fwd[_bf16] (A/B)
namespace sd { void sd_nn_set_pool_pair(int v) { g_pool_pair = v; } }  // (called by sd_set_option in sd_conv.hip)

// the last launch of an entry point: 256 threads per block, check, `return 0` (the macro leaves the function)
#define SD_RETURN_LAUNCH(kernel, grid, lds, st, ...) \
    do { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, st, __VA_ARGS__); SD_LAUNCH_CHECK(); return 0; } while (0)

// ---- launch shapes: what a launcher hands hipLaunchKernelGGL and sd_nn_kernel_names prints (n: the count the kernel is told, where it takes one)
struct Launch { int grid; size_t lds; int64_t n; };
static Launch ew_launch(int64_t n) { return {ew_grid(n), 0, n}; }                                     // grid-stride pass over n groups of elements
static Launch bn_ew_launch(bool wide, int64_t M, int C) { return ew_launch(M * C / (wide ? 8 : 4)); }   // [M][C] in groups of 4, the bf16 x8 kernels of 8
static Launch map_launch(int B, int H, int W, int C, int elems) {                                        // one thread per `elems` channels of a (B, H, W, C) map
    const int64_t n = (int64_t)B * H * W * C / elems;
    return {cdiv(n, 256), 0, n};
}
static Launch pool_fwd_launch(bool pair, int elems, int B, int Ho, int Wo, int C) { return map_launch(B, Ho, Wo, C, pair ? 2 * elems : 4); }
static Launch stem_apply_launch(bool quad, int B, int Hi, int Wi, int C) { return map_launch(B, Hi, Wi, C, quad ? 16 : 4); }   // a quad: 2 x 2 pixels x 4 channels
static Launch chan_launch(int C, int per_block) { return {cdiv(C, per_block), 0, C}; }                 // per channel: 4 a block (the finish), 256 (the tails)
static Launch head_dgrad_launch(int64_t M, int C, int Co) { return {cdiv(M, 64), (size_t)Co * C * sizeof(float), M}; }

// ---- the plan of a column reduction.  Workspace, in floats: [nb partial rows][2][C] | mean(g) (C), mean(g * xhat) (C) of the backward | the
// slab sums of the two-level finish -----------------------------------------------------------------------------------------------------------
enum RowsRule { ROWS_BN, ROWS_STEM_TAIL };
struct FoldPlan { int slab, rows; };                 // slab == 0: no k_rows_fold launch; rows: the rows the finish kernel reads
struct ColReducePlan {
    int rpb, nb;
    FoldPlan fold;
    size_t partial_at, means_at, fold_at;            // float offsets into the workspace
    size_t ws_bytes;
};

// rows per reduction block: 256 for the big maps, fewer for the deep layers so that the pass still spreads over >= 1024 blocks
// (layer4, M = 16384 at bs=64: 64 blocks of 256 rows read at 0.8 TB/s, 1024 blocks of 16 rows at HBM rate)
static int red_rows(int64_t M) {
    int r = RED_ROWS_PER_BLOCK;
    while (r > 16 && M / r < 1024) r >>= 1;
    return r;
}

static int fold_rows(int rows) { return rows > 2048 ? cdiv(rows, std::max(16, rows / 128)) : 0; }      // (<= 2048 rows: one finalize launch is faster)

// Many partial rows: they are folded in coalesced slabs first (a column-slice finalize touches every row from every block), into `scratch`.
static FoldPlan plan_fold(int rows, int C, bool scratch) {
    if (!scratch || fold_rows(rows) == 0 || 2 * C > 1024) return {0, rows};
    const int slab = std::max(16, rows / 128);
    return {slab, cdiv(rows, slab)};
}

// ROWS_STEM_TAIL: the stem tail's kernels take RED_ROWS_PER_BLOCK rows per block whatever M is, while its callers size the workspace with
// sd_col_reduce_workspace_bytes, i.e. by the BatchNorm rule.  That is never the smaller size: red_rows(M) <= RED_ROWS_PER_BLOCK, so the stem
// tail has at most as many partial rows as the BatchNorm rule, and the two differ only for M / 256 < 1024, where neither has rows to fold.
static ColReducePlan plan_col_reduce(int64_t M, int C, RowsRule rule) {
    ColReducePlan p;
    const int nb_bn = cdiv(M, red_rows(M));
    p.rpb = rule == ROWS_STEM_TAIL ? RED_ROWS_PER_BLOCK : red_rows(M);
    p.nb = cdiv(M, p.rpb);
    p.fold = plan_fold(p.nb, C, true);
    p.partial_at = 0;
    p.means_at = (size_t)p.nb * 2 * C;
    p.fold_at = p.means_at + 2 * (size_t)C;
    p.ws_bytes = align_up(((size_t)nb_bn + fold_rows(nb_bn)) * 2 * C * sizeof(float) + 2 * (size_t)C * sizeof(float), 256);
    return p;
}

static const float* launch_fold(const float* partial, int rows, int C, const FoldPlan& f, float* scratch, hipStream_t st) {
    if (!f.slab) return partial;
    hipLaunchKernelGGL(k_rows_fold, dim3(f.rows), dim3(256), 0, st, partial, rows, 2 * C, f.slab, scratch);
    return scratch;
}

// The finish of partial rows [rows][2][C], sums in fp64.  MODE 0: a = mean, b = invstd, c / d = running mean / variance; MODE 1: a = dgamma,
// b = dbeta (+= when accumulate), c / d = mean(g), mean(g * xhat); MODE 2: a = the plain column sums (+=).  With `sums` (synchronized BatchNorm)
// phase 1 only: [S0, S1, n] in fp64 and, MODE 1, dgamma / dbeta from the local sums; the rest then comes from sd_bn_*_from_sums.
template <int MODE>
static void col_finish(const float* fin, int rows, int64_t M, int C, float eps, float momentum, float* a, float* b, float* c, float* d, int accumulate,
                       double* sums, hipStream_t st) {
    float* const none = nullptr;
    if constexpr (MODE != 2) {
        if (sums) {
            hipLaunchKernelGGL(k_col_sums<MODE>, dim3(chan_launch(C, 4).grid), dim3(256), 0, st, fin, rows, C, (double)M, MODE ? a : none, MODE ? b : none, accumulate, sums);
            return;
        }
    }
    hipLaunchKernelGGL(k_col_finalize<MODE>, dim3(chan_launch(C, 4).grid), dim3(256), 0, st, fin, rows, C, (double)M, eps, momentum, a, b, MODE == 0 ? c : none,
                       MODE == 0 ? d : none, MODE == 1 ? c : none, MODE == 1 ? d : none, accumulate);
}

// ---- checkers: one per argument family ------------------------------------------------------------------------------------------------------
static int check_mc(const char* what, int64_t M, int C) {
    SD_REQUIRE(M > 0 && C > 0 && C % 4 == 0 && C <= 1024 && (C / 4) <= 256 && 256 % (C / 4) == 0, SD_ERR_INVALID,
               "%s: needs M > 0 and C in {4..1024} with C/4 dividing 256 (got M=%lld C=%d)", what, (long long)M, C);
    return 0;
}
// the ReLU form of a BatchNorm backward and the pointers it needs: y for the mask from y (1) or the mask bytes (3), beta to recompute it (2)
static int check_relu(const char* what, int relu, const void* y, const void* beta) {
    SD_REQUIRE(relu >= 0 && relu <= 3, SD_ERR_INVALID, "%s: relu must be 0 (none), 1 (mask from y), 2 (mask recomputed from x) or 3 (mask bytes)", what);
    SD_REQUIRE(((relu != 1 && relu != 3) || y) && (relu != 2 || beta), SD_ERR_INVALID, "%s: null pointer", what);
    return 0;
}
static int check_sums(const char* what, const double* sums) {
    SD_REQUIRE((reinterpret_cast<uintptr_t>(sums) & 7u) == 0, SD_ERR_ALIGN, "%s: the fp64 sums must be 8-byte aligned", what);
    return 0;
}
static int check_map(const char* what, bool pointers, int B, int H, int W, int C, int cmul) {
    SD_REQUIRE(pointers && B > 0 && H > 0 && W > 0 && C > 0 && C % cmul == 0, SD_ERR_INVALID, "%s: bad arguments", what);
    return 0;
}
// only the fp32 form of the stem tail's backward has pixel kernels for odd maps
static int check_stem_quad(const char* what, bool quad, bool f32) {
    SD_REQUIRE(quad || f32, SD_ERR_INVALID, "%s: the bf16 form needs even Hi, Wi", what);
    return 0;
}

// ---- predicates: one per kernel choice ------------------------------------------------------------------------------------------------------
// The bf16 x8 kernels of the BatchNorm backward: one choice for the reduce and the apply pass, so that the fused and the split forms reduce
// in the same order.  The reduce-only form has no dx / g_out and passes null (aligned16(nullptr) is true): buffers from one allocator make
// the same choice in both forms.
static bool bn_bwd_wide(int C, int relu, const void* dy, const void* x, const void* dx, const void* g_out) {
    return C % 8 == 0 && relu != 1 && aligned16(dy) && aligned16(x) && aligned16(dx) && aligned16(g_out);
}
static bool bn_apply_wide(int C, const void* x, const void* y, const void* residual) { return C % 8 == 0 && aligned16(x) && aligned16(y) && aligned16(residual); }
// two windows per thread in the stem tail's forward (`option`: pool_fwd_pair; elems channels per thread: 4 fp32, 8 bf16; idx: a byte per channel)
static bool pool_fwd_pair(int option, int elems, int Wo, int C, const void* x, const void* y_pool, const void* idx) {
    return option && Wo % 2 == 0 && C % elems == 0 && aligned16(x) && aligned16(y_pool) && (reinterpret_cast<uintptr_t>(idx) & (uintptr_t)(elems - 1)) == 0;
}
static bool stem_bwd_quad(int Hi, int Wi) { return Hi % 2 == 0 && Wi % 2 == 0; }        // even maps: 2x2 quads share their four windows
// the C = 128 pipelines of the head (the default FPN depth): wave-private LDS-DMA rings
static bool head_fwd_f32_c128(int64_t M, int HW, int C, int Co, const void* x, const void* w, const void* y) {
    return C == 128 && Co <= 16 && HW % 16 == 0 && M < (1ll << 31) && aligned16(x) && aligned16(w) && aligned16(y);
}
static bool head_fwd_bf16_c128(int HW, int C, const void* x, const void* y) { return C == 128 && HW % 4 == 0 && aligned16(x) && aligned16(y); }
static bool head_wgrad_f32_c128(int64_t M, int HW, int C, int Co, const void* x, const void* dy) {
    return C == 128 && Co <= 16 && HW % 16 == 0 && M < (1ll << 31) && aligned16(x) && aligned16(dy);
}

static inline int pool_out(int n) { return (n + 2 - 3) / 2 + 1; }
template <typename... Ts> constexpr bool all_f32 = (std::is_same<Ts, float>::value && ...);
template <typename T> constexpr bool is_bf16 = std::is_same<T, uint16_t>::value;

// ---- BatchNorm and column sums --------------------------------------------------------------------------------------------------------------
// a whole-tensor reduction of x [M][C] through the workspace.  MODE 0: the statistics (sd_bn_train_stats / _sums); 2: sd_col_sum (a = out)
template <int MODE, typename T>
static int col_reduce_any(const char* what, const T* x, int64_t M, int C, float eps, float momentum, float* a, float* b, float* c, float* d, double* sums,
                          int accumulate, void* workspace, size_t workspace_bytes, hipStream_t st) {
    if (int e = check_mc(what, M, C)) return e;
    SD_REQUIRE(x && (MODE == 2 ? a != nullptr : (sums || (a && b))) && workspace, SD_ERR_INVALID, "%s: null pointer", what);
    if (int e = check_sums(what, sums)) return e;
    const ColReducePlan p = plan_col_reduce(M, C, ROWS_BN);
    SD_REQUIRE(workspace_bytes >= p.ws_bytes, SD_ERR_WORKSPACE, "%s: workspace too small", what);
    float* ws = (float*)workspace;
    hipLaunchKernelGGL((k_col_reduce<MODE, T>), dim3(p.nb), dim3(256), 0, st, x, (const T*)nullptr, (const T*)nullptr, (const float*)nullptr,
                       (const float*)nullptr, (const float*)nullptr, (const float*)nullptr, 0, M, C, ws + p.partial_at, p.rpb);
    SD_LAUNCH_CHECK();
    const float* fin = launch_fold(ws + p.partial_at, p.nb, C, p.fold, ws + p.fold_at, st);
    col_finish<MODE>(fin, p.fold.rows, M, C, eps, momentum, a, b, c, d, accumulate, sums, st);
    SD_LAUNCH_CHECK();
    return 0;
}

// The reduction half of sd_bn_bwd[_bf16]: partial rows of (sum g, sum g * xhat) into the workspace, then the finish (the two means at the
// plan's means_at, or with `sums` phase 1 into the caller's fp64 buffer).  `wide`: bn_bwd_wide, the caller's choice.  `plan_out`: where a fused
// form finds the means.
template <typename T>
static int bn_bwd_reduce_any(const char* what, const T* dy, const T* x, const void* y, int relu, int64_t M, int C, const float* mean,
                             const float* invstd, const float* gamma, const float* beta, float* dgamma, float* dbeta, int accumulate,
                             double* sums, bool wide, void* workspace, size_t workspace_bytes, hipStream_t st, ColReducePlan* plan_out = nullptr) {
    if (int e = check_mc(what, M, C)) return e;
    if (int e = check_relu(what, relu, y, beta)) return e;
    SD_REQUIRE(dy && x && mean && invstd && gamma && dgamma && dbeta && workspace, SD_ERR_INVALID, "%s: null pointer", what);
    if (int e = check_sums(what, sums)) return e;
    const ColReducePlan p = plan_col_reduce(M, C, ROWS_BN);
    SD_REQUIRE(workspace_bytes >= p.ws_bytes, SD_ERR_WORKSPACE, "%s: workspace too small", what);
    float* ws = (float*)workspace;
    float* partial = ws + p.partial_at;
    if (is_bf16<T> && wide)
        hipLaunchKernelGGL(k_col_reduce_bwd_bf16x8, dim3(p.nb), dim3(256), 0, st, (const uint16_t*)dy, (const uint16_t*)x, (const uint8_t*)y, mean, invstd,
                           gamma, beta, relu, M, C, partial, p.rpb);
    else
        hipLaunchKernelGGL((k_col_reduce<1, T>), dim3(p.nb), dim3(256), 0, st, dy, x, (const T*)y, mean, invstd, gamma, beta, relu, M, C, partial, p.rpb);
    SD_LAUNCH_CHECK();
    const float* fin = launch_fold(partial, p.nb, C, p.fold, ws + p.fold_at, st);
    col_finish<1>(fin, p.fold.rows, M, C, 0.f, 0.f, dgamma, dbeta, ws + p.means_at, ws + p.means_at + C, accumulate, sums, st);
    SD_LAUNCH_CHECK();
    if (plan_out) *plan_out = p;
    return 0;
}

// the apply pass of the BatchNorm backward (means = [mean(g) (C), mean(g * xhat) (C)])
template <typename T>
static int bn_bwd_apply_launch(const T* dy, const T* x, const void* y, int relu, int64_t M, int C, const float* mean, const float* invstd,
                               const float* gamma, const float* beta, const float* means, T* dx, T* g_out, bool wide, hipStream_t st) {
    const Launch l = bn_ew_launch(is_bf16<T> && wide, M, C);
    if (is_bf16<T> && wide)
        SD_RETURN_LAUNCH(k_bn_bwd_apply_bf16x8, l.grid, 0, st, (const uint16_t*)dy, (const uint16_t*)x, (const uint8_t*)y, relu, l.n, C, mean, invstd, gamma,
                      beta, means, means + C, (uint16_t*)dx, (uint16_t*)g_out);
    SD_RETURN_LAUNCH(k_bn_bwd_apply<T>, l.grid, 0, st, dy, x, (const T*)y, relu, l.n, C, mean, invstd, gamma, beta, means, means + C, dx, g_out);
}

template <typename T>
static int bn_bwd_any(const char* what, const T* dy, const T* x, const void* y, int relu, int64_t M, int C, const float* mean, const float* invstd,
                      const float* gamma, const float* beta, T* dx, T* g_out, float* dgamma, float* dbeta, int accumulate, void* workspace,
                      size_t workspace_bytes, hipStream_t st) {
    SD_REQUIRE(dx, SD_ERR_INVALID, "%s: null pointer", what);
    const bool wide = is_bf16<T> && bn_bwd_wide(C, relu, dy, x, dx, g_out);
    ColReducePlan p;
    if (int e = bn_bwd_reduce_any<T>(what, dy, x, y, relu, M, C, mean, invstd, gamma, beta, dgamma, dbeta, accumulate, nullptr, wide, workspace,
                                     workspace_bytes, st, &p)) return e;
    return bn_bwd_apply_launch<T>(dy, x, y, relu, M, C, mean, invstd, gamma, beta, (const float*)workspace + p.means_at, dx, g_out, wide, st);
}

template <typename T>
static int bn_bwd_apply_any(const char* what, const T* dy, const T* x, const void* y, int relu, int64_t M, int C, const float* mean,
                            const float* invstd, const float* gamma, const float* beta, const float* means, T* dx, T* g_out, hipStream_t st) {
    if (int e = check_mc(what, M, C)) return e;
    if (int e = check_relu(what, relu, y, beta)) return e;
    SD_REQUIRE(dy && x && mean && invstd && gamma && means && dx, SD_ERR_INVALID, "%s: null pointer", what);
    return bn_bwd_apply_launch<T>(dy, x, y, relu, M, C, mean, invstd, gamma, beta, means, dx, g_out, is_bf16<T> && bn_bwd_wide(C, relu, dy, x, dx, g_out), st);
}

// frozen BatchNorm, backward: the vector kernel where every pointer given is 16-byte aligned (null counts as aligned; bf16: and C % 8 == 0)
static bool frozen_bwd_wide(bool bf16, int C, const void* dy, const void* y, const void* dx, const void* g_out) {
    return (!bf16 || C % 8 == 0) && aligned16(dy) && aligned16(y) && aligned16(dx) && aligned16(g_out);
}
static Launch frozen_bwd_launch(bool bf16, bool wide, int64_t M, int C) { return ew_launch(wide ? M * C / (bf16 ? 8 : 4) : M * C); }
static bool ranges_meet(const void* a, const void* b, size_t bytes) {                 // two buffers of `bytes` each share a byte (null: no buffer)
    const uintptr_t p = reinterpret_cast<uintptr_t>(a), q = reinterpret_cast<uintptr_t>(b);
    return a && b && p < q + bytes && q < p + bytes;
}

template <typename T>
static int bn_frozen_bwd_any(const char* what, const T* dy, const T* y, const float* scale, int64_t M, int C, T* dx, T* g_out, hipStream_t st) {
    if (int e = check_mc(what, M, C)) return e;
    SD_REQUIRE(dy && scale && dx, SD_ERR_INVALID, "%s: null pointer", what);
    const size_t bytes = (size_t)M * C * sizeof(T);
    SD_REQUIRE(!ranges_meet(dx, dy, bytes) && !ranges_meet(dx, y, bytes) && !ranges_meet(g_out, dy, bytes) && !ranges_meet(g_out, y, bytes) &&
               !ranges_meet(dx, g_out, bytes), SD_ERR_INVALID, "%s: dx and g_out must not alias dy, y or each other", what);
    const bool wide = frozen_bwd_wide(is_bf16<T>, C, dy, y, dx, g_out);
    const Launch l = frozen_bwd_launch(is_bf16<T>, wide, M, C);
    if (!wide) SD_RETURN_LAUNCH(k_bn_frozen_bwd_ew<T>, l.grid, 0, st, dy, y, scale, l.n, C, dx, g_out);
    if constexpr (is_bf16<T>) SD_RETURN_LAUNCH(k_bn_frozen_bwd_bf16x8, l.grid, 0, st, dy, y, scale, l.n, C, dx, g_out);
    else SD_RETURN_LAUNCH(k_bn_frozen_bwd_f32x4, l.grid, 0, st, dy, y, scale, l.n, C, dx, g_out);
}

// The finish on caller-provided partial rows [rows][2][C] (one per conv tile: up to 8192), MODE and a..d as col_finish.  `split`: phase 1 of
// synchronized BatchNorm into `sums` -- same rows, scratch and summation order as the one-launch form.
template <int MODE>
static int rows_finish_any(const char* what, bool split, const float* partial, int rows, int64_t M, int C, float eps, float momentum, float* a, float* b,
                           float* c, float* d, int accumulate, double* sums, float* scratch, hipStream_t st) {
    if (int e = check_mc(what, M, C)) return e;
    const bool outputs = split ? sums && (MODE == 0 || (a && b)) : a && b && (MODE == 0 || c);
    SD_REQUIRE(partial && outputs && rows > 0, SD_ERR_INVALID,
               split ? "%s: bad arguments (null pointer or rows <= 0)" : "%s: bad arguments", what);
    if (int e = check_sums(what, sums)) return e;
    const FoldPlan f = plan_fold(rows, C, scratch != nullptr);
    const float* fin = launch_fold(partial, rows, C, f, scratch, st);
    SD_LAUNCH_CHECK();
    col_finish<MODE>(fin, f.rows, M, C, eps, momentum, a, b, c, d, accumulate, sums, st);
    SD_LAUNCH_CHECK();
    return 0;
}

template <typename T>
static int bn_apply_any(const char* what, const T* x, T* y, int64_t M, int C, const float* mean, const float* invstd, const float* gamma,
                        const float* beta, const T* residual, int relu, uint8_t* relu_mask_out, hipStream_t st) {
    if (int e = check_mc(what, M, C)) return e;
    SD_REQUIRE(x && y && mean && invstd && gamma && beta, SD_ERR_INVALID, "%s: null pointer", what);
    const bool wide = is_bf16<T> && bn_apply_wide(C, x, y, residual);
    const Launch l = bn_ew_launch(wide, M, C);
    if (wide)
        SD_RETURN_LAUNCH(k_bn_apply_bf16x8, l.grid, 0, st, (const uint16_t*)x, (uint16_t*)y, l.n, C, mean, invstd, gamma, beta, (const uint16_t*)residual, relu,
                      relu_mask_out);
    SD_RETURN_LAUNCH(k_bn_apply<T>, l.grid, 0, st, x, y, l.n, C, mean, invstd, gamma, beta, residual, relu, relu_mask_out);
}

// ---- pooling, the stem tail, upsample -------------------------------------------------------------------------------------------------------
template <typename T>
static int bn_relu_maxpool_fwd_any(const char* what, const T* x, int B, int Hi, int Wi, int C, const float* mean, const float* invstd,
                                   const float* gamma, const float* beta, T* y_pool, uint8_t* idx, hipStream_t st) {
    if (int e = check_map(what, x && mean && invstd && gamma && beta && y_pool && idx, B, Hi, Wi, C, 4)) return e;
    constexpr int ELEMS = is_bf16<T> ? 8 : 4;
    const int Ho = pool_out(Hi), Wo = pool_out(Wi);
    const bool pair = pool_fwd_pair(g_pool_pair, ELEMS, Wo, C, x, y_pool, idx);
    const Launch l = pool_fwd_launch(pair, ELEMS, B, Ho, Wo, C);
    if (pair) SD_RETURN_LAUNCH((k_bn_relu_maxpool_fwd_pair<T, T, ELEMS>), l.grid, 0, st, x, mean, invstd, gamma, beta, y_pool, idx, B, Hi, Wi, Ho, Wo, C);
    SD_RETURN_LAUNCH((k_bn_relu_maxpool_fwd<T, T>), l.grid, 0, st, x, mean, invstd, gamma, beta, y_pool, idx, B, Hi, Wi, Ho, Wo, C);
}

// The stem tail's backward (max-pool -> ReLU -> BatchNorm): reduce, finish, apply.  Split forms for synchronized BatchNorm: `sums` -> stop
// after phase 1 (dgamma / dbeta from the local sums, [S0, S1, n] in fp64); the apply pass alone takes the means.  `fused`: called by the fused
// form, which has checked the map already.
template <typename XT>
static int stem_bwd_reduce_any(const char* what, bool fused, const XT* dpool, const uint8_t* idx, const XT* x, int B, int Hi, int Wi, int C,
                               const float* mean, const float* invstd, const float* gamma, const float* beta, float* dgamma, float* dbeta,
                               int accumulate, double* sums, void* workspace, size_t workspace_bytes, hipStream_t st, ColReducePlan* plan_out = nullptr) {
    const int64_t M = (int64_t)B * Hi * Wi;
    if (int e = check_mc(what, M, C)) return e;
    SD_REQUIRE(dpool && idx && x && mean && invstd && gamma && beta && dgamma && dbeta && workspace, SD_ERR_INVALID, "%s: null pointer", what);
    if (int e = check_sums(what, sums)) return e;
    const ColReducePlan p = plan_col_reduce(M, C, ROWS_STEM_TAIL);
    SD_REQUIRE(workspace_bytes >= p.ws_bytes, SD_ERR_WORKSPACE, "%s: workspace too small", what);
    const bool quad = stem_bwd_quad(Hi, Wi);
    if (!fused) if (int e = check_stem_quad(what, quad, all_f32<XT>)) return e;
    const int Ho = pool_out(Hi), Wo = pool_out(Wi);
    float* ws = (float*)workspace;
    float* partial = ws + p.partial_at;
    if (quad) hipLaunchKernelGGL((k_pool_bn_bwd_reduce_quad<XT, XT>), dim3(p.nb), dim3(256), 0, st, dpool, idx, x, mean, invstd, gamma, beta, Hi, Wi, Ho, Wo, M / 4, C, partial);
    else if constexpr (all_f32<XT>) hipLaunchKernelGGL(k_pool_bn_bwd_reduce, dim3(p.nb), dim3(256), 0, st, dpool, idx, x, mean, invstd, gamma, beta, Hi, Wi, Ho, Wo, M, C, partial);
    SD_LAUNCH_CHECK();
    const float* fin = launch_fold(partial, p.nb, C, p.fold, ws + p.fold_at, st);
    col_finish<1>(fin, p.fold.rows, M, C, 0.f, 0.f, dgamma, dbeta, ws + p.means_at, ws + p.means_at + C, accumulate, sums, st);
    SD_LAUNCH_CHECK();
    if (plan_out) *plan_out = p;
    return 0;
}

template <typename XT, typename DT>
static int stem_bwd_apply_launch(const XT* dpool, const uint8_t* idx, const XT* x, int B, int Hi, int Wi, int C, const float* mean, const float* invstd,
                                 const float* gamma, const float* beta, const float* means, DT* dx, hipStream_t st) {
    const int Ho = pool_out(Hi), Wo = pool_out(Wi);
    const bool quad = stem_bwd_quad(Hi, Wi);
    const Launch l = stem_apply_launch(quad, B, Hi, Wi, C);
    if (quad)
        SD_RETURN_LAUNCH((k_pool_bn_bwd_apply_quad<XT, XT, DT>), l.grid, 0, st, dpool, idx, x, mean, invstd, gamma, beta, means, means + C, Hi, Wi, Ho, Wo, l.n,
                      C, dx);
    if constexpr (all_f32<XT, DT>)
        SD_RETURN_LAUNCH(k_pool_bn_bwd_apply, l.grid, 0, st, dpool, idx, x, mean, invstd, gamma, beta, means, means + C, Hi, Wi, Ho, Wo, l.n, C, dx);
    return 0;                                        // (a bf16 form on an odd map: refused by check_stem_quad before it gets here)
}

template <typename XT, typename DT>
static int stem_bwd_apply_any(const char* what, const XT* dpool, const uint8_t* idx, const XT* x, int B, int Hi, int Wi, int C, const float* mean,
                              const float* invstd, const float* gamma, const float* beta, const float* means, DT* dx, hipStream_t st) {
    if (int e = check_mc(what, (int64_t)B * Hi * Wi, C)) return e;
    SD_REQUIRE(dpool && idx && x && mean && invstd && gamma && beta && means && dx, SD_ERR_INVALID, "%s: null pointer", what);
    if (int e = check_stem_quad(what, stem_bwd_quad(Hi, Wi), all_f32<XT, DT>)) return e;
    return stem_bwd_apply_launch<XT, DT>(dpool, idx, x, B, Hi, Wi, C, mean, invstd, gamma, beta, means, dx, st);
}

template <typename XT, typename DT>
static int stem_bwd_any(const char* what, const XT* dpool, const uint8_t* idx, const XT* x, int B, int Hi, int Wi, int C, const float* mean,
                        const float* invstd, const float* gamma, const float* beta, DT* dx, float* dgamma, float* dbeta, int accumulate,
                        void* workspace, size_t workspace_bytes, hipStream_t st) {
    SD_REQUIRE(dx, SD_ERR_INVALID, "%s: null pointer", what);
    if (int e = check_stem_quad(what, stem_bwd_quad(Hi, Wi), all_f32<XT, DT>)) return e;
    ColReducePlan p;
    if (int e = stem_bwd_reduce_any<XT>(what, true, dpool, idx, x, B, Hi, Wi, C, mean, invstd, gamma, beta, dgamma, dbeta, accumulate, nullptr, workspace,
                                        workspace_bytes, st, &p)) return e;
    return stem_bwd_apply_launch<XT, DT>(dpool, idx, x, B, Hi, Wi, C, mean, invstd, gamma, beta, (const float*)workspace + p.means_at, dx, st);
}

template <typename T>
static int upsample2x_bwd_any(const char* what, const T* dy, const T* add, T* dx, int B, int H, int W, int C, hipStream_t st) {
    if (int e = check_map(what, dy && dx, B, H, W, C, 4)) return e;
    SD_RETURN_LAUNCH(k_up2_bwd<T>, map_launch(B, H, W, C, 4).grid, 0, st, dy, add, dx, B, H, W, C);
}

// ---- the narrow head (Co <= HEAD_NARROW_MAX_CO; wider ones: sd_head_wide.hip) ---------------------------------------------------------------
struct HeadLaunch { bool c128; int grid, rows; size_t lds; };             // rows: tiles of the forward, partial rows of the weight gradient

static HeadLaunch plan_head_fwd(bool bf16, int64_t M, int HW, int C, int Co, const void* x, const void* w, const void* y) {
    if (bf16 && head_fwd_bf16_c128(HW, C, x, y)) {                         // wave-private LDS-DMA + bf16 MFMA pipeline
        const int ntiles = cdiv(M, 64);
        return {true, std::max(1, std::min(cdiv(ntiles, 4), 1024)), ntiles, 0};
    }
    if (!bf16 && head_fwd_f32_c128(M, HW, C, Co, x, w, y)) {
        const int ntiles = (int)(M / 16);
        return {true, std::min(cdiv(ntiles, 4), 256), ntiles, (size_t)4 * HF_NST * 2048 * sizeof(float)};
    }
    return {false, cdiv(M, 64), 0, ((size_t)64 * (C + 4) + (size_t)Co * C) * sizeof(float)};
}

// partial rows of the head weight gradient: one per block of k_head_wgrad[_bf16] (HEAD_WG_PIX pixels), or one per WAVE of k_head_wgrad_f32_c128
// (up to 1024 waves = one block of four waves per CU, each wave on tiles of 16 pixels)
static HeadLaunch plan_head_wgrad(bool c128, int64_t M) {
    if (!c128) return {false, cdiv(M, HEAD_WG_PIX), cdiv(M, HEAD_WG_PIX), 0};
    const int rows = (int)std::min<int64_t>(1024, (cdiv(M, 16) + 3) / 4 * 4);
    return {true, rows / 4, rows, (size_t)4 * HF_NST * HWG_STAGE * sizeof(float)};
}

static inline int head_fin_grid(int C, int Co) { return cdiv(Co * C + Co, 8); }
static void head_wgrad_fin(const float* partial, int rows, int C, int Co, float* dw, float* dbias, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(k_head_wgrad_fin, dim3(head_fin_grid(C, Co)), dim3(256), 0, st, partial, rows, Co * C + Co, dw, dbias, Co * C, accumulate);
}

// the dynamic LDS of a C = 128 pipeline is above the default limit: raised once per process, at the kernel's first launch
#define SD_RAISE_LDS_ONCE(kernel, bytes)                                                                                                               \
    static const hipError_t attr_once = hipFuncSetAttribute(reinterpret_cast<const void*>(&kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)(bytes)); \
    SD_HIP(attr_once)

// ---- the optimizer --------------------------------------------------------------------------------------------------------------------------
static int adam_launch(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n4, float lr, float beta1, float beta2, float eps,
                       double bc1, double bc2, float grad_scale, hipStream_t st) {
    SD_RETURN_LAUNCH(k_adam, ew_launch(n4).grid, 0, st, param, grad, exp_avg, exp_avg_sq, n4, lr, beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), grad_scale);
}

static inline int sumsq_blocks(int64_t n) { return n > 0 ? (int)std::min<int64_t>(cdiv(n / 4, 256), SUMSQ_MAX_BLOCKS) : 0; }

// ==== the C ABI.  The fp32 and bf16 forms of an entry point are one template body behind two exported names: FORMS stamps the export (NAME,
// element type T, and V = the element type the C prototype shows: float, or void for bf16) ====================================================
extern "C" {

size_t sd_col_reduce_workspace_bytes(int64_t M, int C) { return plan_col_reduce(M, C, ROWS_BN).ws_bytes; }
// rows of `scratch` the two-level finish of `rows` partial rows needs (0 = single level)
int sd_bn_finalize_scratch_rows(int rows) { return fold_rows(rows); }

#define FORMS(NAME, T, V)                                                                                                                               \
    int NAME(const V* x, int64_t M, int C, float eps, float momentum, float* running_mean, float* running_var, float* mean, float* invstd, void* workspace, \
             size_t workspace_bytes, sd_stream_t stream) {                                                                                              \
        return col_reduce_any<0, T>(#NAME, (const T*)x, M, C, eps, momentum, mean, invstd, running_mean, running_var, nullptr, 0, workspace, workspace_bytes, \
                                    (hipStream_t)stream);                                                                                               \
    }
FORMS(sd_bn_train_stats, float, float)
FORMS(sd_bn_train_stats_bf16, uint16_t, void)
#undef FORMS

// synchronized BatchNorm: the statistics up to sums = [S0 = sum x (C), S1 = sum x^2 (C), n = M] in fp64 (sd_bn_stats_from_sums finishes)
#define FORMS(NAME, T, V)                                                                                                                          \
    int NAME(const V* x, int64_t M, int C, double* sums, void* workspace, size_t workspace_bytes, sd_stream_t stream) {                            \
        SD_REQUIRE(sums, SD_ERR_INVALID, #NAME ": null sums");                                                                                     \
        return col_reduce_any<0, T>(#NAME, (const T*)x, M, C, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr, sums, 0, workspace, workspace_bytes,  \
                                    (hipStream_t)stream);                                                                                          \
    }
FORMS(sd_bn_train_sums, float, float)
FORMS(sd_bn_train_sums_bf16, uint16_t, void)
#undef FORMS

#define FORMS(NAME, T, V)                                                                                                                           \
    int NAME(const V* x, int64_t M, int C, float* out, int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream) {              \
        return col_reduce_any<2, T>(#NAME, (const T*)x, M, C, 0.f, 0.f, out, nullptr, nullptr, nullptr, nullptr, accumulate, workspace, workspace_bytes, \
                                    (hipStream_t)stream);                                                                                           \
    }
FORMS(sd_col_sum, float, float)
FORMS(sd_col_sum_bf16, uint16_t, void)
#undef FORMS

int sd_bn_finalize_stats(const float* partial, int rows, int64_t M, int C, float eps, float momentum, float* running_mean,
                         float* running_var, float* mean, float* invstd, float* scratch, sd_stream_t stream) {
    return rows_finish_any<0>("sd_bn_finalize_stats", false, partial, rows, M, C, eps, momentum, mean, invstd, running_mean, running_var, 0, nullptr,
                              scratch, (hipStream_t)stream);
}

// synchronized BatchNorm, forward: phase 1 of sd_bn_finalize_stats; after any all-reduce of `sums`, sd_bn_stats_from_sums finishes
int sd_bn_stats_sums(const float* partial, int rows, int64_t M, int C, double* sums, float* scratch, sd_stream_t stream) {
    return rows_finish_any<0>("sd_bn_stats_sums", true, partial, rows, M, C, 0.f, 0.f, nullptr, nullptr, nullptr, nullptr, 0, sums, scratch,
                              (hipStream_t)stream);
}

// second half of the reduction of sd_bn_bwd on caller-provided partial rows (sum g, sum g * xhat): dgamma / dbeta (+=) and
// means_out = [mean(g) (C), mean(g * xhat) (C)] for sd_bn_bwd_apply
int sd_bn_bwd_finalize(const float* partial, int rows, int64_t M, int C, float* dgamma, float* dbeta, int accumulate, float* means_out,
                       float* scratch, sd_stream_t stream) {
    return rows_finish_any<1>("sd_bn_bwd_finalize", false, partial, rows, M, C, 0.f, 0.f, dgamma, dbeta, means_out, means_out ? means_out + C : nullptr,
                              accumulate, nullptr, scratch, (hipStream_t)stream);
}

// synchronized BatchNorm, backward: phase 1 of sd_bn_bwd_finalize -- dgamma / dbeta (+=) from the local sums and
// sums = [sum g (C), sum g * xhat (C), n = M] in fp64
int sd_bn_bwd_sums(const float* partial, int rows, int64_t M, int C, float* dgamma, float* dbeta, int accumulate, double* sums, float* scratch,
                   sd_stream_t stream) {
    return rows_finish_any<1>("sd_bn_bwd_sums", true, partial, rows, M, C, 0.f, 0.f, dgamma, dbeta, nullptr, nullptr, accumulate, sums, scratch,
                              (hipStream_t)stream);
}

// phase 2: mean, invstd (biased variance) and the running statistics (unbiased with n = sums[2C]) from [S0, S1, n]
int sd_bn_stats_from_sums(const double* sums, int C, float eps, float momentum, float* running_mean, float* running_var, float* mean,
                          float* invstd, sd_stream_t stream) {
    if (int e = check_mc("sd_bn_stats_from_sums", 1, C)) return e;
    SD_REQUIRE(sums && mean && invstd && (running_mean != nullptr) == (running_var != nullptr), SD_ERR_INVALID,
               "sd_bn_stats_from_sums: null pointer (running_mean and running_var are both given or both null)");
    if (int e = check_sums("sd_bn_stats_from_sums", sums)) return e;
    SD_RETURN_LAUNCH(k_bn_stats_from_sums, chan_launch(C, 256).grid, 0, (hipStream_t)stream, sums, C, eps, momentum, mean, invstd, running_mean, running_var);
}

// phase 2: means_out = [S0 / n (C), S1 / n (C)] with n = sums[2C], what sd_bn_bwd_apply[_bf16] / sd_maxpool_bn_relu_bwd_apply* consume
int sd_bn_bwd_means_from_sums(const double* sums, int C, float* means_out, sd_stream_t stream) {
    if (int e = check_mc("sd_bn_bwd_means_from_sums", 1, C)) return e;
    SD_REQUIRE(sums && means_out, SD_ERR_INVALID, "sd_bn_bwd_means_from_sums: null pointer");
    if (int e = check_sums("sd_bn_bwd_means_from_sums", sums)) return e;
    SD_RETURN_LAUNCH(k_bn_bwd_means_from_sums, chan_launch(C, 256).grid, 0, (hipStream_t)stream, sums, C, means_out);
}

// bf16 activations (mixed-precision training): the same kernels with 2-byte loads / stores, all arithmetic in fp32
#define FORMS(NAME, T, V)                                                                                                                          \
    int NAME(const V* x, V* y, int64_t M, int C, const float* mean, const float* invstd, const float* gamma, const float* beta, const V* residual, \
             int relu, uint8_t* relu_mask_out, sd_stream_t stream) {                                                                               \
        return bn_apply_any<T>(#NAME, (const T*)x, (T*)y, M, C, mean, invstd, gamma, beta, (const T*)residual, relu, relu_mask_out, (hipStream_t)stream); \
    }
FORMS(sd_bn_apply, float, float)
FORMS(sd_bn_apply_bf16, uint16_t, void)
#undef FORMS

int sd_bn_fold(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps, int C, float* scale,
               float* shift, sd_stream_t stream) {
    SD_REQUIRE(gamma && beta && running_mean && running_var && scale && shift && C > 0, SD_ERR_INVALID, "sd_bn_fold: bad arguments");
    SD_RETURN_LAUNCH(k_bn_fold, chan_launch(C, 256).grid, 0, (hipStream_t)stream, gamma, beta, running_mean, running_var, eps, C, scale, shift);
}

#define FORMS(NAME, T, V)                                                                                                                            \
    int NAME(const V* dy, const V* x, const V* y, int relu, int64_t M, int C, const float* mean, const float* invstd, const float* gamma,            \
             const float* beta, V* dx, V* g_out, float* dgamma, float* dbeta, int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream) { \
        return bn_bwd_any<T>(#NAME, (const T*)dy, (const T*)x, y, relu, M, C, mean, invstd, gamma, beta, (T*)dx, (T*)g_out, dgamma, dbeta, accumulate, \
                             workspace, workspace_bytes, (hipStream_t)stream);                                                                       \
    }
FORMS(sd_bn_bwd, float, float)
FORMS(sd_bn_bwd_bf16, uint16_t, void)
#undef FORMS

// synchronized BatchNorm, backward: the reduce half of sd_bn_bwd alone -- dgamma / dbeta (+=) from the local sums and
// sums = [sum g (C), sum g * xhat (C), n = M] in fp64; after any all-reduce of `sums`, sd_bn_bwd_means_from_sums + sd_bn_bwd_apply
#define FORMS(NAME, T, V)                                                                                                                             \
    int NAME(const V* dy, const V* x, const V* y, int relu, int64_t M, int C, const float* mean, const float* invstd, const float* gamma,             \
             const float* beta, float* dgamma, float* dbeta, int accumulate, double* sums, void* workspace, size_t workspace_bytes, sd_stream_t stream) { \
        SD_REQUIRE(sums, SD_ERR_INVALID, #NAME ": null pointer");                                                                                     \
        return bn_bwd_reduce_any<T>(#NAME, (const T*)dy, (const T*)x, y, relu, M, C, mean, invstd, gamma, beta, dgamma, dbeta, accumulate, sums,      \
                                    is_bf16<T> && bn_bwd_wide(C, relu, dy, x, nullptr, nullptr), workspace, workspace_bytes, (hipStream_t)stream);    \
    }
FORMS(sd_bn_bwd_reduce, float, float)
FORMS(sd_bn_bwd_reduce_bf16, uint16_t, void)
#undef FORMS

// apply pass of sd_bn_bwd with the two per-channel means already known (sd_conv2d_dgrad_bn_reduce / sd_bn_bwd_finalize / ..._from_sums)
#define FORMS(NAME, T, V)                                                                                                                          \
    int NAME(const V* dy, const V* x, const V* y, int relu, int64_t M, int C, const float* mean, const float* invstd, const float* gamma,          \
             const float* beta, const float* means, V* dx, V* g_out, sd_stream_t stream) {                                                         \
        return bn_bwd_apply_any<T>(#NAME, (const T*)dy, (const T*)x, y, relu, M, C, mean, invstd, gamma, beta, means, (T*)dx, (T*)g_out, (hipStream_t)stream); \
    }
FORMS(sd_bn_bwd_apply, float, float)
FORMS(sd_bn_bwd_apply_bf16, uint16_t, void)
#undef FORMS

// backward of a BatchNorm that normalises with its stored statistics (scale: sd_bn_fold's): no reduction, one pass
#define FORMS(NAME, T, V)                                                                                                              \
    int NAME(const V* dy, const V* y, const float* scale, int64_t M, int C, V* dx, V* g_out, sd_stream_t stream) {                    \
        return bn_frozen_bwd_any<T>(#NAME, (const T*)dy, (const T*)y, scale, M, C, (T*)dx, (T*)g_out, (hipStream_t)stream);            \
    }
FORMS(sd_frozen_bn_bwd, float, float)
FORMS(sd_frozen_bn_bwd_bf16, uint16_t, void)
#undef FORMS

int sd_maxpool3x3s2_fwd(const float* x, float* y, uint8_t* idx, int B, int Hi, int Wi, int C, sd_stream_t stream) {
    if (int e = check_map("sd_maxpool3x3s2_fwd", x && y && idx, B, Hi, Wi, C, 4)) return e;
    const int Ho = pool_out(Hi), Wo = pool_out(Wi);
    SD_RETURN_LAUNCH(k_maxpool_fwd, map_launch(B, Ho, Wo, C, 4).grid, 0, (hipStream_t)stream, x, y, idx, B, Hi, Wi, Ho, Wo, C);
}

int sd_maxpool3x3s2_fwd_bf16(const void* x, void* y, int B, int Hi, int Wi, int C, sd_stream_t stream) {
    if (int e = check_map("sd_maxpool3x3s2_fwd_bf16", x && y, B, Hi, Wi, C, 8)) return e;
    const int Ho = pool_out(Hi), Wo = pool_out(Wi);
    SD_RETURN_LAUNCH(k_maxpool_fwd_bf16, map_launch(B, Ho, Wo, C, 8).grid, 0, (hipStream_t)stream, (const uint16_t*)x, (uint16_t*)y, B, Hi, Wi, Ho, Wo, C);
}

int sd_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, float* dx, int B, int Hi, int Wi, int C, sd_stream_t stream) {
    if (int e = check_map("sd_maxpool3x3s2_bwd", dy && dx && idx, B, Hi, Wi, C, 4)) return e;
    SD_RETURN_LAUNCH(k_maxpool_bwd, map_launch(B, Hi, Wi, C, 4).grid, 0, (hipStream_t)stream, dy, idx, dx, B, Hi, Wi, pool_out(Hi), pool_out(Wi), C);
}

#define FORMS(NAME, T, V)                                                                                                                     \
    int NAME(const V* x, int B, int Hi, int Wi, int C, const float* mean, const float* invstd, const float* gamma, const float* beta, V* y_pool, \
             uint8_t* idx, sd_stream_t stream) {                                                                                              \
        return bn_relu_maxpool_fwd_any<T>(#NAME, (const T*)x, B, Hi, Wi, C, mean, invstd, gamma, beta, (T*)y_pool, idx, (hipStream_t)stream); \
    }
FORMS(sd_bn_relu_maxpool_fwd, float, float)
FORMS(sd_bn_relu_maxpool_fwd_bf16, uint16_t, void)
#undef FORMS

// the stem tail's backward: fp32; bf16 pooled gradient and conv output with an fp32 dx; the same with a bf16 dx (what sd_conv2d_stem_wgrad_bf16
// reads: under autocast the stem conv's output gradient is bf16).  T / V: the inputs, DT / DV: dx
#define FORMS(NAME, T, V, DT, DV)                                                                                                                    \
    int NAME(const V* dpool, const uint8_t* idx, const V* x, int B, int Hi, int Wi, int C, const float* mean, const float* invstd, const float* gamma, \
             const float* beta, DV* dx, float* dgamma, float* dbeta, int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream) {  \
        return stem_bwd_any<T, DT>(#NAME, (const T*)dpool, idx, (const T*)x, B, Hi, Wi, C, mean, invstd, gamma, beta, (DT*)dx, dgamma, dbeta, accumulate, \
                                   workspace, workspace_bytes, (hipStream_t)stream);                                                                 \
    }
FORMS(sd_maxpool_bn_relu_bwd, float, float, float, float)
FORMS(sd_maxpool_bn_relu_bwd_bf16, uint16_t, void, float, float)
FORMS(sd_maxpool_bn_relu_bwd_bf16_dx16, uint16_t, void, uint16_t, void)
#undef FORMS

// synchronized BatchNorm: its reduce half (dgamma / dbeta += local sums; [S0, S1, n] fp64 into `sums`) ...
#define FORMS(NAME, T, V)                                                                                                                            \
    int NAME(const V* dpool, const uint8_t* idx, const V* x, int B, int Hi, int Wi, int C, const float* mean, const float* invstd, const float* gamma, \
             const float* beta, float* dgamma, float* dbeta, int accumulate, double* sums, void* workspace, size_t workspace_bytes, sd_stream_t stream) { \
        SD_REQUIRE(sums, SD_ERR_INVALID, #NAME ": null pointer");                                                                                    \
        return stem_bwd_reduce_any<T>(#NAME, false, (const T*)dpool, idx, (const T*)x, B, Hi, Wi, C, mean, invstd, gamma, beta, dgamma, dbeta, accumulate, \
                                      sums, workspace, workspace_bytes, (hipStream_t)stream);                                                        \
    }
FORMS(sd_maxpool_bn_relu_bwd_reduce, float, float)
FORMS(sd_maxpool_bn_relu_bwd_reduce_bf16, uint16_t, void)
#undef FORMS

// ... and the apply pass from the two means of sd_bn_bwd_means_from_sums
#define FORMS(NAME, T, V, DT, DV)                                                                                                                    \
    int NAME(const V* dpool, const uint8_t* idx, const V* x, int B, int Hi, int Wi, int C, const float* mean, const float* invstd, const float* gamma, \
             const float* beta, const float* means, DV* dx, sd_stream_t stream) {                                                                    \
        return stem_bwd_apply_any<T, DT>(#NAME, (const T*)dpool, idx, (const T*)x, B, Hi, Wi, C, mean, invstd, gamma, beta, means, (DT*)dx, (hipStream_t)stream); \
    }
FORMS(sd_maxpool_bn_relu_bwd_apply, float, float, float, float)
FORMS(sd_maxpool_bn_relu_bwd_apply_bf16, uint16_t, void, float, float)
FORMS(sd_maxpool_bn_relu_bwd_apply_bf16_dx16, uint16_t, void, uint16_t, void)
#undef FORMS

#define FORMS(NAME, T, V)                                                                                                  \
    int NAME(const V* dy, const V* add, V* dx, int B, int H, int W, int C, sd_stream_t stream) {                          \
        return upsample2x_bwd_any<T>(#NAME, (const T*)dy, (const T*)add, (T*)dx, B, H, W, C, (hipStream_t)stream);        \
    }
FORMS(sd_upsample2x_bwd, float, float)
FORMS(sd_upsample2x_bwd_bf16, uint16_t, void)
#undef FORMS

int sd_cast_f32_to_bf16(const float* x, void* y, int64_t n, sd_stream_t stream) {
    SD_REQUIRE(x && y && n > 0 && n % 4 == 0 && aligned16(x), SD_ERR_INVALID, "sd_cast_f32_to_bf16: bad arguments (n %% 4 == 0, 16-byte aligned source)");
    SD_RETURN_LAUNCH(k_cast_bf16, ew_launch(n / 4).grid, 0, (hipStream_t)stream, x, (uint16_t*)y, n / 4);
}

int sd_cast_bf16_to_f32(const void* x, float* y, int64_t n, sd_stream_t stream) {
    SD_REQUIRE(x && y && n > 0 && n % 4 == 0 && aligned16(y) && (reinterpret_cast<uintptr_t>(x) & 7u) == 0, SD_ERR_INVALID,
               "sd_cast_bf16_to_f32: bad arguments (n %% 4 == 0, 8-byte aligned source, 16-byte aligned destination)");
    SD_RETURN_LAUNCH(k_cast_f32, ew_launch(n / 4).grid, 0, (hipStream_t)stream, (const uint16_t*)x, y, n / 4);
}

int sd_head_fwd_bf16(const void* x, const float* w, const float* bias, float* y, int B, int HW, int C, int Co, sd_stream_t stream) {
    SD_REQUIRE(x && w && bias && y && B > 0 && HW > 0, SD_ERR_INVALID, "sd_head_fwd_bf16: bad arguments");
    if (Co > HEAD_NARROW_MAX_CO) return head_wide_fwd_bf16(x, w, bias, y, B, HW, C, Co, (hipStream_t)stream);    // sd_head_wide.hip
    SD_REQUIRE(C % 8 == 0 && C <= 512 && Co > 0 && Co <= HEAD_NARROW_MAX_CO, SD_ERR_INVALID, "sd_head_fwd_bf16: needs C %% 8 == 0, C <= 512, Co <= %d", HEAD_NARROW_MAX_CO);
    const int64_t M = (int64_t)B * HW;
    const HeadLaunch l = plan_head_fwd(true, M, HW, C, Co, x, w, y);
    if (l.c128 && Co <= 16) SD_RETURN_LAUNCH(k_head_fwd_bf16_c128<false>, l.grid, 0, (hipStream_t)stream, (const uint16_t*)x, w, bias, y, M, HW, Co, l.rows);
    if (l.c128) SD_RETURN_LAUNCH(k_head_fwd_bf16_c128<true>, l.grid, 0, (hipStream_t)stream, (const uint16_t*)x, w, bias, y, M, HW, Co, l.rows);
    SD_RETURN_LAUNCH(k_head_fwd_bf16, l.grid, l.lds, (hipStream_t)stream, (const uint16_t*)x, w, bias, y, M, HW, C, Co);
}

int sd_head_fwd(const float* x, const float* w, const float* bias, float* y, int B, int HW, int C, int Co, sd_stream_t stream) {
    SD_REQUIRE(x && w && bias && y && B > 0 && HW > 0, SD_ERR_INVALID, "sd_head_fwd: bad arguments");
    if (Co > HEAD_NARROW_MAX_CO) return head_wide_fwd(x, w, bias, y, B, HW, C, Co, (hipStream_t)stream);              // sd_head_wide.hip
    SD_REQUIRE(C % 4 == 0 && C <= 512 && Co > 0 && Co <= HEAD_NARROW_MAX_CO, SD_ERR_INVALID, "sd_head_fwd: needs C %% 4 == 0, C <= 512, Co <= %d", HEAD_NARROW_MAX_CO);
    const int64_t M = (int64_t)B * HW;
    const HeadLaunch l = plan_head_fwd(false, M, HW, C, Co, x, w, y);
    if (l.c128) {
        SD_RAISE_LDS_ONCE(k_head_fwd_f32_c128, l.lds);
        SD_RETURN_LAUNCH(k_head_fwd_f32_c128, l.grid, l.lds, (hipStream_t)stream, x, w, bias, y, HW, Co, l.rows);
    }
    SD_RETURN_LAUNCH(k_head_fwd, l.grid, l.lds, (hipStream_t)stream, x, w, bias, y, M, HW, C, Co);
}

// the narrow head sizes for the larger of its two weight-gradient kernels: the pointers that choose between them are not known here
size_t sd_head_bwd_workspace_bytes(int B, int HW, int C, int Co) {
    const int64_t M = (int64_t)B * HW;
    if (Co > HEAD_NARROW_MAX_CO) return head_wide_bwd_workspace_bytes(M, C, Co);
    return align_up((size_t)std::max(plan_head_wgrad(false, M).rows, plan_head_wgrad(true, M).rows) * (Co * C + Co) * sizeof(float), 256);
}

int sd_head_bwd(const float* dy, const float* x, const float* w, float* dx, float* dw, float* dbias, int B, int HW, int C, int Co,
                int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_REQUIRE(dy && x && w && dx && dw && dbias && workspace && B > 0 && HW > 0, SD_ERR_INVALID, "sd_head_bwd: bad arguments");
    const int64_t M = (int64_t)B * HW;
    hipStream_t st = (hipStream_t)stream;
    if (Co > HEAD_NARROW_MAX_CO) {                                             // GEMM kernels of sd_head_wide.hip
        if (int e = head_wide_check("sd_head_bwd", M, C, Co)) return e;
        SD_REQUIRE(workspace_bytes >= sd_head_bwd_workspace_bytes(B, HW, C, Co), SD_ERR_WORKSPACE, "sd_head_bwd: workspace too small");
        int rows = 0;
        if (int e = head_wide_wgrad(dy, x, (float*)workspace, B, HW, C, Co, st, rows)) return e;
        head_wgrad_fin((const float*)workspace, rows, C, Co, dw, dbias, accumulate, st);
        SD_LAUNCH_CHECK();
        return head_wide_dgrad(dy, w, dx, B, HW, C, Co, st);
    }
    SD_REQUIRE(C % 4 == 0 && C <= 256 && (256 % C == 0) && (64 % (256 / C) == 0) && ((64 / (256 / C)) % 8 == 0) && Co > 0 && Co <= HEAD_NARROW_MAX_CO,
               SD_ERR_INVALID, "sd_head_bwd: needs C in {64, 128, 256} and Co <= %d", HEAD_NARROW_MAX_CO);
    SD_REQUIRE(workspace_bytes >= sd_head_bwd_workspace_bytes(B, HW, C, Co), SD_ERR_WORKSPACE, "sd_head_bwd: workspace too small");
    // weight gradient first: it streams x while HBM is quiet; behind the data-gradient it shared the memory system with the write-back
    // of that kernel's 537 MB (144 us instead of ~105)
    const HeadLaunch l = plan_head_wgrad(head_wgrad_f32_c128(M, HW, C, Co, x, dy), M);
    if (l.c128) {
        SD_RAISE_LDS_ONCE(k_head_wgrad_f32_c128, l.lds);
        hipLaunchKernelGGL(k_head_wgrad_f32_c128, dim3(l.grid), dim3(256), l.lds, st, dy, x, (float*)workspace, HW, Co, (int)(M / 16));
    } else {
        hipLaunchKernelGGL(k_head_wgrad, dim3(l.grid), dim3(256), 0, st, dy, x, (float*)workspace, M, HW, C, Co);
    }
    SD_LAUNCH_CHECK();
    head_wgrad_fin((const float*)workspace, l.rows, C, Co, dw, dbias, accumulate, st);
    SD_LAUNCH_CHECK();
    const Launch dg = head_dgrad_launch(M, C, Co);
    SD_RETURN_LAUNCH(k_head_dgrad<float>, dg.grid, dg.lds, st, dy, w, dx, M, HW, C, Co);
}

int sd_head_bwd_bf16(const float* dy, const void* x_bf16, const float* w, void* dx_bf16, float* dw, float* dbias, int B, int HW, int C, int Co,
                     int accumulate, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_REQUIRE(dy && x_bf16 && w && dx_bf16 && dw && dbias && workspace && B > 0 && HW > 0, SD_ERR_INVALID, "sd_head_bwd_bf16: bad arguments");
    SD_REQUIRE((C == 64 || C == 128) && Co > 0 && Co <= 8, SD_ERR_INVALID, "sd_head_bwd_bf16: needs C in {64, 128} and Co <= 8 (got %d, %d)", C, Co);
    SD_REQUIRE(aligned16(x_bf16) && aligned16(dx_bf16), SD_ERR_ALIGN, "sd_head_bwd_bf16: x and dx must be 16-byte aligned");
    SD_REQUIRE(workspace_bytes >= sd_head_bwd_workspace_bytes(B, HW, C, Co), SD_ERR_WORKSPACE, "sd_head_bwd_bf16: workspace too small");
    const int64_t M = (int64_t)B * HW;
    hipStream_t st = (hipStream_t)stream;
    const Launch dg = head_dgrad_launch(M, C, Co);
    hipLaunchKernelGGL(k_head_dgrad<uint16_t>, dim3(dg.grid), dim3(256), dg.lds, st, dy, w, (uint16_t*)dx_bf16, M, HW, C, Co);
    SD_LAUNCH_CHECK();
    const HeadLaunch l = plan_head_wgrad(false, M);
    hipLaunchKernelGGL(k_head_wgrad_bf16<8>, dim3(l.grid), dim3(256), 0, st, dy, (const uint16_t*)x_bf16, (float*)workspace, M, HW, C, Co);
    SD_LAUNCH_CHECK();
    head_wgrad_fin((const float*)workspace, l.rows, C, Co, dw, dbias, accumulate, st);
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr, float beta1, float beta2,
                 float eps, float grad_scale, sd_stream_t stream) {
    SD_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && n % 4 == 0 && step >= 1, SD_ERR_INVALID, "sd_adam_step: bad arguments (n %% 4 == 0, step >= 1)");
    SD_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq), SD_ERR_ALIGN, "sd_adam_step: pointers must be 16-byte aligned");
    return adam_launch(param, grad, exp_avg, exp_avg_sq, n / 4, lr, beta1, beta2, eps, 1.0 - pow((double)beta1, step), 1.0 - pow((double)beta2, step),
                       grad_scale, (hipStream_t)stream);
}

size_t sd_grad_sumsq_workspace_bytes(int64_t n) { return (size_t)sumsq_blocks(n) * sizeof(double); }

int sd_grad_sumsq(const float* grad, int64_t n, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_REQUIRE(grad && workspace && n > 0 && n % 4 == 0, SD_ERR_INVALID, "sd_grad_sumsq: bad arguments (n %% 4 == 0)");
    SD_REQUIRE(aligned16(grad) && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, SD_ERR_ALIGN,
               "sd_grad_sumsq: grad must be 16-byte aligned, the workspace 8-byte aligned");
    SD_REQUIRE(workspace_bytes >= sd_grad_sumsq_workspace_bytes(n), SD_ERR_WORKSPACE, "sd_grad_sumsq: workspace too small");
    SD_RETURN_LAUNCH(k_grad_sumsq, sumsq_blocks(n), 0, (hipStream_t)stream, grad, n / 4, (double*)workspace);
}

int sd_optim_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr, float beta1, float beta2,
                  float eps, float grad_scale, float weight_decay, const uint8_t* decay_mask, float max_norm, const void* partials,
                  int npartials, float* ema, float ema_decay, void* status, sd_stream_t stream) {
    SD_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && n % 4 == 0 && step >= 1, SD_ERR_INVALID, "sd_optim_step: bad arguments (n %% 4 == 0, step >= 1)");
    SD_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(ema), SD_ERR_ALIGN,
               "sd_optim_step: pointers must be 16-byte aligned");
    SD_REQUIRE(weight_decay >= 0.f, SD_ERR_INVALID, "sd_optim_step: weight_decay must be >= 0 (got %g)", (double)weight_decay);
    SD_REQUIRE(max_norm >= 0.f, SD_ERR_INVALID, "sd_optim_step: max_norm must be >= 0 (got %g; 0 = no clipping)", (double)max_norm);
    SD_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, SD_ERR_INVALID, "sd_optim_step: ema_decay must be in [0, 1) (got %g)", (double)ema_decay);
    const bool decay = weight_decay > 0.f, clip = max_norm > 0.f, avg = ema != nullptr;
    if (clip) {
        SD_REQUIRE(partials && npartials > 0 && status, SD_ERR_INVALID,
                   "sd_optim_step: max_norm > 0 needs the partials of sd_grad_sumsq (pointer and count) and the status block");
        SD_REQUIRE(npartials == sumsq_blocks(n), SD_ERR_INVALID, "sd_optim_step: %d partials, sd_grad_sumsq writes %d for n = %lld "
                   "(sd_grad_sumsq_workspace_bytes(n) / 8)", npartials, sumsq_blocks(n), (long long)n);
        SD_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0, SD_ERR_ALIGN,
                   "sd_optim_step: partials must be 8-byte aligned, the status block 4-byte aligned");
    }
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const int64_t n4 = n / 4;
    if (!decay && !clip && !avg)                                               // every option off: sd_adam_step's own launch
        return adam_launch(param, grad, exp_avg, exp_avg_sq, n4, lr, beta1, beta2, eps, bc1, bc2, grad_scale, (hipStream_t)stream);
    using kernel_t = decltype(&k_optim<true, true, true>);
    static const kernel_t variants[8] = {nullptr,                      k_optim<true, false, false>, k_optim<false, true, false>,
                                         k_optim<true, true, false>,   k_optim<false, false, true>, k_optim<true, false, true>,
                                         k_optim<false, true, true>,   k_optim<true, true, true>};
    const float decay_mul = (float)(1.0 - (double)lr * (double)weight_decay);
    SD_RETURN_LAUNCH(variants[(int)decay | (int)clip << 1 | (int)avg << 2], ew_launch(n4).grid, 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n4, lr, beta1,
                  beta2, eps, (float)bc1, (float)sqrt(bc2), grad_scale, decay_mul, decay_mask, max_norm, (const double*)partials, npartials, ema, ema_decay,
                  (uint32_t*)status);
}

int sd_optim_groups_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr, float beta1, float beta2,
                         float eps, float grad_scale, float weight_decay, const uint8_t* group_ids, const float* lr_mul, const float* wd_mul,
                         int ngroups, float max_norm, const void* partials, int npartials, float* ema, float ema_decay, void* status,
                         sd_stream_t stream) {
    SD_REQUIRE(param && grad && exp_avg && exp_avg_sq && n > 0 && n % 4 == 0 && step >= 1, SD_ERR_INVALID,
               "sd_optim_groups_step: bad arguments (n %% 4 == 0, step >= 1)");
    SD_REQUIRE(group_ids && lr_mul && wd_mul, SD_ERR_INVALID, "sd_optim_groups_step: needs group_ids (device, n / 4 bytes) and the host arrays lr_mul and wd_mul");
    SD_REQUIRE(ngroups >= 1 && ngroups <= SD_OPTIM_MAX_GROUPS, SD_ERR_INVALID, "sd_optim_groups_step: ngroups must be in [1, %d] (got %d)",
               SD_OPTIM_MAX_GROUPS, ngroups);
    SD_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(ema), SD_ERR_ALIGN,
               "sd_optim_groups_step: pointers must be 16-byte aligned");
    SD_REQUIRE(weight_decay >= 0.f, SD_ERR_INVALID, "sd_optim_groups_step: weight_decay must be >= 0 (got %g)", (double)weight_decay);
    SD_REQUIRE(max_norm >= 0.f, SD_ERR_INVALID, "sd_optim_groups_step: max_norm must be >= 0 (got %g; 0 = no clipping)", (double)max_norm);
    SD_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, SD_ERR_INVALID, "sd_optim_groups_step: ema_decay must be in [0, 1) (got %g)", (double)ema_decay);
    for (int k = 0; k < ngroups; ++k) {
        SD_REQUIRE(std::isfinite(lr_mul[k]) && lr_mul[k] >= 0.f, SD_ERR_INVALID, "sd_optim_groups_step: lr_mul[%d] must be finite and >= 0 (got %g)", k,
                   (double)lr_mul[k]);
        SD_REQUIRE(std::isfinite(wd_mul[k]) && wd_mul[k] >= 0.f, SD_ERR_INVALID, "sd_optim_groups_step: wd_mul[%d] must be finite and >= 0 (got %g)", k,
                   (double)wd_mul[k]);
    }
    const bool clip = max_norm > 0.f, avg = ema != nullptr;
    if (clip) {
        SD_REQUIRE(partials && npartials > 0 && status, SD_ERR_INVALID,
                   "sd_optim_groups_step: max_norm > 0 needs the partials of sd_grad_sumsq (pointer and count) and the status block");
        SD_REQUIRE(npartials == sumsq_blocks(n), SD_ERR_INVALID, "sd_optim_groups_step: %d partials, sd_grad_sumsq writes %d for n = %lld "
                   "(sd_grad_sumsq_workspace_bytes(n) / 8)", npartials, sumsq_blocks(n), (long long)n);
        SD_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0, SD_ERR_ALIGN,
                   "sd_optim_groups_step: partials must be 8-byte aligned, the status block 4-byte aligned");
    }
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    OptimGroupTable tab;
    uint32_t decay_bits = 0;
    for (int k = 0; k < SD_OPTIM_MAX_GROUPS; ++k) {                            // rows past ngroups: a group that does not move
        const float lr_k = k < ngroups ? lr * lr_mul[k] : 0.f;
        const bool decay = k < ngroups && weight_decay > 0.f && wd_mul[k] > 0.f;
        // k_optim divides `lr / bc1` in fp32 on the device; this is the same division on the host.  The two agree bit for bit because both
        // are IEEE correctly rounded: hipcc's default for fp32 division (this file is built without fast-math or a relaxed-division flag).
        tab.step[k] = lr_k / (float)bc1;
        tab.decay_mul[k] = decay ? (float)(1.0 - (double)lr_k * (double)weight_decay * (double)wd_mul[k]) : 1.f;
        decay_bits |= (uint32_t)decay << k;
    }
    using kernel_t = decltype(&k_optim_groups<true, true>);
    static const kernel_t variants[4] = {k_optim_groups<false, false>, k_optim_groups<true, false>, k_optim_groups<false, true>, k_optim_groups<true, true>};
    const int64_t n4 = n / 4;
    SD_RETURN_LAUNCH(variants[(int)clip | (int)avg << 1], ew_launch(n4).grid, 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n4, tab, decay_bits,
                     beta1, beta2, eps, (float)sqrt(bc2), grad_scale, group_ids, max_norm, (const double*)partials, npartials, ema, ema_decay,
                     (uint32_t*)status);
}

// ---- sd_sgd_step / sd_lamb_step: the groups form's checks, said once for both (sd_optim_groups_step's refusals and codes) ----------------
static int check_groups_form(const char* what, const void* param, const void* grad, int64_t n, float weight_decay, const uint8_t* group_ids,
                             const float* lr_mul, const float* wd_mul, int ngroups, float max_norm, const void* partials, int npartials,
                             const void* ema, float ema_decay, const void* status) {
    SD_REQUIRE(param && grad && n > 0 && n % 4 == 0, SD_ERR_INVALID, "%s: bad arguments (null param / grad, n > 0, n %% 4 == 0)", what);
    SD_REQUIRE(group_ids && lr_mul && wd_mul, SD_ERR_INVALID, "%s: needs group_ids (device, n / 4 bytes) and the host arrays lr_mul and wd_mul", what);
    SD_REQUIRE(ngroups >= 1 && ngroups <= SD_OPTIM_MAX_GROUPS, SD_ERR_INVALID, "%s: ngroups must be in [1, %d] (got %d)", what, SD_OPTIM_MAX_GROUPS, ngroups);
    SD_REQUIRE(aligned16(param) && aligned16(grad) && aligned16(ema), SD_ERR_ALIGN, "%s: pointers must be 16-byte aligned", what);
    SD_REQUIRE(weight_decay >= 0.f && std::isfinite(weight_decay), SD_ERR_INVALID, "%s: weight_decay must be finite and >= 0 (got %g)", what, (double)weight_decay);
    SD_REQUIRE(max_norm >= 0.f, SD_ERR_INVALID, "%s: max_norm must be >= 0 (got %g; 0 = no clipping)", what, (double)max_norm);
    SD_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, SD_ERR_INVALID, "%s: ema_decay must be in [0, 1) (got %g)", what, (double)ema_decay);
    for (int k = 0; k < ngroups; ++k) {
        SD_REQUIRE(std::isfinite(lr_mul[k]) && lr_mul[k] >= 0.f, SD_ERR_INVALID, "%s: lr_mul[%d] must be finite and >= 0 (got %g)", what, k, (double)lr_mul[k]);
        SD_REQUIRE(std::isfinite(wd_mul[k]) && wd_mul[k] >= 0.f, SD_ERR_INVALID, "%s: wd_mul[%d] must be finite and >= 0 (got %g)", what, k, (double)wd_mul[k]);
    }
    if (max_norm > 0.f) {
        SD_REQUIRE(partials && npartials > 0 && status, SD_ERR_INVALID,
                   "%s: max_norm > 0 needs the partials of sd_grad_sumsq (pointer and count) and the status block", what);
        SD_REQUIRE(npartials == sumsq_blocks(n), SD_ERR_INVALID, "%s: %d partials, sd_grad_sumsq writes %d for n = %lld "
                   "(sd_grad_sumsq_workspace_bytes(n) / 8)", what, npartials, sumsq_blocks(n), (long long)n);
        SD_REQUIRE((reinterpret_cast<uintptr_t>(partials) & 7u) == 0 && (reinterpret_cast<uintptr_t>(status) & 3u) == 0, SD_ERR_ALIGN,
                   "%s: partials must be 8-byte aligned, the status block 4-byte aligned", what);
    }
    return 0;
}

// lr_k = lr * lr_mul[k], wd_k = weight_decay * wd_mul[k] (one fp32 multiply each); rows past ngroups: a group that does not move
static SgdGroupTable rate_table(float lr, float weight_decay, const float* lr_mul, const float* wd_mul, int ngroups) {
    SgdGroupTable tab;
    for (int k = 0; k < SD_OPTIM_MAX_GROUPS; ++k) {
        tab.lr[k] = k < ngroups ? lr * lr_mul[k] : 0.f;
        tab.wd[k] = k < ngroups ? weight_decay * wd_mul[k] : 0.f;
    }
    return tab;
}

int sd_sgd_step(float* param, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum, int nesterov, float grad_scale,
                float weight_decay, const uint8_t* group_ids, const float* lr_mul, const float* wd_mul, int ngroups, float max_norm,
                const void* partials, int npartials, float* ema, float ema_decay, void* status, sd_stream_t stream) {
    if (int e = check_groups_form("sd_sgd_step", param, grad, n, weight_decay, group_ids, lr_mul, wd_mul, ngroups, max_norm, partials, npartials, ema,
                                  ema_decay, status)) return e;
    SD_REQUIRE(momentum >= 0.f && momentum < 1.f, SD_ERR_INVALID, "sd_sgd_step: momentum must be in [0, 1) (got %g)", (double)momentum);
    SD_REQUIRE(nesterov == 0 || nesterov == 1, SD_ERR_INVALID, "sd_sgd_step: nesterov must be 0 or 1 (got %d)", nesterov);
    SD_REQUIRE(!nesterov || momentum > 0.f, SD_ERR_INVALID, "sd_sgd_step: nesterov needs momentum > 0");
    SD_REQUIRE(momentum == 0.f || momentum_buf, SD_ERR_INVALID, "sd_sgd_step: momentum > 0 needs the momentum buffer (bad arguments)");
    SD_REQUIRE(aligned16(momentum_buf), SD_ERR_ALIGN, "sd_sgd_step: pointers must be 16-byte aligned");
    const SgdGroupTable tab = rate_table(lr, weight_decay, lr_mul, wd_mul, ngroups);
    const bool clip = max_norm > 0.f, avg = ema != nullptr;
    const int64_t n4 = n / 4;
    const int mom = momentum == 0.f ? 0 : nesterov ? 2 : 1;                    // one kernel per (momentum kind, clipping, EMA)
    using kernel_t = decltype(&k_sgd<0, true, true>);
    static const kernel_t variants[12] = {k_sgd<0, false, false>, k_sgd<0, true, false>, k_sgd<0, false, true>, k_sgd<0, true, true>,
                                          k_sgd<1, false, false>, k_sgd<1, true, false>, k_sgd<1, false, true>, k_sgd<1, true, true>,
                                          k_sgd<2, false, false>, k_sgd<2, true, false>, k_sgd<2, false, true>, k_sgd<2, true, true>};
    SD_RETURN_LAUNCH(variants[4 * mom | (int)clip | (int)avg << 1], ew_launch(n4).grid, 0, (hipStream_t)stream, param, grad, mom ? momentum_buf : nullptr, n4,
                     tab, momentum, grad_scale, group_ids, max_norm, (const double*)partials, npartials, ema, ema_decay, (uint32_t*)status);
}

// ---- LAMB's slot table (host only) -------------------------------------------------------------------------------------------------------
static int lamb_slot_blocks(int64_t floats) { return (int)std::min<int64_t>(cdiv(floats, SD_LAMB_BLOCK_FLOATS), SD_LAMB_MAX_SLOT_BLOCKS); }

size_t sd_lamb_workspace_bytes(int nblocks) { return nblocks > 0 ? (size_t)nblocks * 2 * sizeof(double) : 0; }

int sd_lamb_table_build(const int64_t* slot_lo, const int64_t* slot_hi, const uint8_t* adapt, int nslots, int64_t n, void* table, size_t table_bytes,
                        size_t* bytes_needed, int* nblocks) {
    SD_REQUIRE(slot_lo && slot_hi && adapt, SD_ERR_INVALID, "sd_lamb_table_build: needs the host arrays slot_lo, slot_hi and adapt");
    SD_REQUIRE(nslots >= 1 && nslots <= SD_LAMB_MAX_SLOTS, SD_ERR_INVALID, "sd_lamb_table_build: nslots must be in [1, %d] (got %d)", SD_LAMB_MAX_SLOTS, nslots);
    SD_REQUIRE(n > 0 && n % 8 == 0 && n / 4 <= INT32_MAX, SD_ERR_INVALID, "sd_lamb_table_build: n must be a positive multiple of 8 below 2^33 (got %lld)",
               (long long)n);
    int64_t at = 0, blocks = 0;
    for (int s = 0; s < nslots; ++s) {
        SD_REQUIRE(slot_lo[s] == at && slot_hi[s] > slot_lo[s] && slot_hi[s] <= n && slot_hi[s] % 8 == 0, SD_ERR_INVALID,
                   "sd_lamb_table_build: slot %d is [%lld, %lld): the slots must tile [0, n) in order, each a positive multiple of 8 floats "
                   "(expected it to start at %lld; n = %lld)", s, (long long)slot_lo[s], (long long)slot_hi[s], (long long)at, (long long)n);
        at = slot_hi[s];
        blocks += lamb_slot_blocks(slot_hi[s] - slot_lo[s]);
    }
    SD_REQUIRE(at == n, SD_ERR_INVALID, "sd_lamb_table_build: the slots end at %lld, the buffer at n = %lld", (long long)at, (long long)n);
    const size_t need = ((size_t)nslots * 4 + (size_t)blocks) * sizeof(int32_t);
    if (bytes_needed) *bytes_needed = need;
    if (nblocks) *nblocks = (int)blocks;
    if (!table) return 0;                                                      // the size query
    SD_REQUIRE(table_bytes >= need, SD_ERR_WORKSPACE, "sd_lamb_table_build: the table needs %zu bytes (got %zu)", need, table_bytes);
    int32_t* rows = (int32_t*)table;
    int32_t* owner = rows + 4 * (size_t)nslots;
    int first = 0;
    for (int s = 0; s < nslots; ++s) {
        const int nb = lamb_slot_blocks(slot_hi[s] - slot_lo[s]);
        rows[4 * s] = (int32_t)(slot_lo[s] / 4);
        rows[4 * s + 1] = (int32_t)(slot_hi[s] / 4);
        rows[4 * s + 2] = first;
        rows[4 * s + 3] = nb | (adapt[s] ? 1 << 30 : 0);
        for (int b = 0; b < nb; ++b) owner[first + b] = s;
        first += nb;
    }
    return 0;
}

int sd_lamb_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, int step, float lr, float beta1, float beta2,
                 float eps, float grad_scale, float weight_decay, const uint8_t* group_ids, const float* lr_mul, const float* wd_mul, int ngroups,
                 float max_norm, const void* partials, int npartials, float* ema, float ema_decay, void* status, const void* table, int nslots,
                 int nblocks, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    if (int e = check_groups_form("sd_lamb_step", param, grad, n, weight_decay, group_ids, lr_mul, wd_mul, ngroups, max_norm, partials, npartials, ema,
                                  ema_decay, status)) return e;
    SD_REQUIRE(exp_avg && exp_avg_sq && step >= 1, SD_ERR_INVALID, "sd_lamb_step: bad arguments (null exp_avg / exp_avg_sq, step >= 1)");
    SD_REQUIRE(aligned16(exp_avg) && aligned16(exp_avg_sq), SD_ERR_ALIGN, "sd_lamb_step: pointers must be 16-byte aligned");
    SD_REQUIRE(n / 4 <= INT32_MAX, SD_ERR_INVALID, "sd_lamb_step: n must be below 2^33 (got %lld)", (long long)n);
    SD_REQUIRE(table && workspace, SD_ERR_INVALID, "sd_lamb_step: needs the slot table (device, from sd_lamb_table_build) and the workspace");
    SD_REQUIRE(nslots >= 1 && nslots <= SD_LAMB_MAX_SLOTS, SD_ERR_INVALID, "sd_lamb_step: nslots must be in [1, %d] (got %d)", SD_LAMB_MAX_SLOTS, nslots);
    SD_REQUIRE(nblocks >= nslots && (int64_t)nblocks <= (int64_t)nslots * SD_LAMB_MAX_SLOT_BLOCKS, SD_ERR_INVALID,
               "sd_lamb_step: nblocks must be in [nslots, %d * nslots] (got %d for %d slots)", SD_LAMB_MAX_SLOT_BLOCKS, nblocks, nslots);
    SD_REQUIRE(aligned16(table) && (reinterpret_cast<uintptr_t>(workspace) & 7u) == 0, SD_ERR_ALIGN,
               "sd_lamb_step: the table must be 16-byte aligned, the workspace 8-byte aligned");
    SD_REQUIRE(workspace_bytes >= sd_lamb_workspace_bytes(nblocks), SD_ERR_WORKSPACE, "sd_lamb_step: workspace too small (%zu bytes, %d blocks need %zu)",
               workspace_bytes, nblocks, sd_lamb_workspace_bytes(nblocks));
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    const SgdGroupTable tab = rate_table(lr, weight_decay, lr_mul, wd_mul, ngroups);
    const bool clip = max_norm > 0.f, avg = ema != nullptr;
    const int64_t n4 = n / 4;
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(clip ? k_lamb_moments<true> : k_lamb_moments<false>, dim3(nblocks), dim3(256), 0, st, param, grad, exp_avg, exp_avg_sq, n4, tab, beta1,
                       beta2, eps, (float)bc1, (float)sqrt(bc2), grad_scale, group_ids, max_norm, (const double*)partials, npartials, (uint32_t*)status,
                       (const int32_t*)table, nslots, nblocks, (double*)workspace);
    SD_LAUNCH_CHECK();
    using kernel_t = decltype(&k_lamb_apply<true, true>);
    static const kernel_t variants[4] = {k_lamb_apply<false, false>, k_lamb_apply<true, false>, k_lamb_apply<false, true>, k_lamb_apply<true, true>};
    SD_RETURN_LAUNCH(variants[(int)clip | (int)avg << 1], nblocks, 0, st, param, exp_avg, exp_avg_sq, n4, tab, eps, (float)bc1, (float)sqrt(bc2), grad_scale,
                     group_ids, max_norm, (const double*)partials, npartials, ema, ema_decay, (const int32_t*)table, nslots, nblocks,
                     (const double*)workspace);
}

// the count and the mode of sd_grad_accum (shared with sd_nn_kernel_names)
static int check_grad_accum(const char* what, int64_t n, int overwrite) {
    SD_REQUIRE(n >= 0 && n % 4 == 0, SD_ERR_INVALID, "%s: needs n >= 0 and n %% 4 == 0 (got %lld)", what, (long long)n);
    SD_REQUIRE(overwrite == 0 || overwrite == 1, SD_ERR_INVALID, "%s: overwrite must be 0 (add) or 1 (copy), got %d", what, overwrite);
    return 0;
}

int sd_grad_accum(float* dst, const float* src, int64_t n, int overwrite, sd_stream_t stream) {
    if (int e = check_grad_accum("sd_grad_accum", n, overwrite)) return e;
    if (n == 0) return 0;                                                     // an empty range (a stage that is frozen whole): no launch
    SD_REQUIRE(dst && src, SD_ERR_INVALID, "sd_grad_accum: null pointer");
    SD_REQUIRE(aligned16(dst) && aligned16(src), SD_ERR_ALIGN, "sd_grad_accum: pointers must be 16-byte aligned");
    const uintptr_t d = reinterpret_cast<uintptr_t>(dst), s = reinterpret_cast<uintptr_t>(src), bytes = (uintptr_t)n * sizeof(float);
    SD_REQUIRE(d == s || d + bytes <= s || s + bytes <= d, SD_ERR_INVALID,
               "sd_grad_accum: dst and src overlap without being the same range (in place on dst: every group of four is read, then written)");
    const Launch l = ew_launch(n / 4);
    if (overwrite) SD_RETURN_LAUNCH(k_grad_accum<true>, l.grid, 0, (hipStream_t)stream, dst, src, l.n);
    SD_RETURN_LAUNCH(k_grad_accum<false>, l.grid, 0, (hipStream_t)stream, dst, src, l.n);
}

// ---- sd_nn_kernel_names: the plans above, printed (host only; the one place of this layer that formats) -------------------------------------
namespace {
struct Names {
    char* buf; size_t cap, at;
    void put(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
        va_list ap;
        va_start(ap, fmt);
        if (at < cap) at += vsnprintf(buf + at, cap - at, fmt, ap);
        va_end(ap);
    }
    void add(const char* name, int64_t grid, size_t lds = 0) { put("%s%s grid=%lld block=256 lds=%zu", at ? "; " : "", name, (long long)grid, lds); }
    void add(const char* name, const Launch& l) { add(name, l.grid, l.lds); }
    void reduce(const char* kernel, int nb, const FoldPlan& f, int mode, bool sums, int C) {      // the launches of every reducing op
        char fin[32];
        snprintf(fin, sizeof(fin), sums ? "k_col_sums<%d>" : "k_col_finalize<%d>", mode);
        if (kernel) add(kernel, nb);
        if (f.slab) add("k_rows_fold", f.rows);
        add(fin, chan_launch(C, 4));
    }
    void plan(const ColReducePlan& p) {
        put(" | rpb=%d nb=%d slab=%d rows=%d partial_at=%zu means_at=%zu fold_at=%zu ws_bytes=%zu", p.rpb, p.nb, p.fold.slab, p.fold.rows, p.partial_at,
            p.means_at, p.fold_at, p.ws_bytes);
    }
};
}  // namespace

// the shapes the entry points refuse, by their checkers
static int check_desc(const char* what, const sd_nn_call_desc& d, int64_t M) {
    switch (d.op) {
    case SD_NN_BN_STATS_FROM_SUMS: case SD_NN_BN_BWD_MEANS_FROM_SUMS: return check_mc(what, 1, d.C);
    case SD_NN_BN_TRAIN_STATS: case SD_NN_BN_FINALIZE_STATS: case SD_NN_BN_APPLY: case SD_NN_BN_BWD_FINALIZE: case SD_NN_COL_SUM: case SD_NN_BN_FROZEN_BWD:
        return check_mc(what, M, d.C);
    case SD_NN_BN_BWD: case SD_NN_BN_BWD_REDUCE: case SD_NN_BN_BWD_APPLY:
        if (int e = check_mc(what, M, d.C)) return e;
        return check_relu(what, d.relu, what, what);
    case SD_NN_MAXPOOL_FWD: case SD_NN_MAXPOOL_BWD: case SD_NN_BN_RELU_MAXPOOL_FWD: case SD_NN_UPSAMPLE_BWD:
        return check_map(what, true, d.B, d.H, d.W, d.C, d.op == SD_NN_MAXPOOL_FWD && d.form ? 8 : 4);
    case SD_NN_STEM_BWD: case SD_NN_STEM_BWD_REDUCE: case SD_NN_STEM_BWD_APPLY:
        if (int e = check_stem_quad(what, stem_bwd_quad(d.H, d.W), !d.form)) return e;
        return check_mc(what, M, d.C);
    case SD_NN_CAST: case SD_NN_ADAM: case SD_NN_GRAD_SUMSQ: case SD_NN_OPTIM: case SD_NN_OPTIM_GROUPS: case SD_NN_SGD: case SD_NN_LAMB:
        SD_REQUIRE(M > 0 && M % 4 == 0, SD_ERR_INVALID, "%s: needs n > 0 and n %% 4 == 0 (got %lld)", what, (long long)M);
        SD_REQUIRE(d.op != SD_NN_SGD || (d.form >= 0 && d.form <= 2), SD_ERR_INVALID, "%s: sgd's form must be 0 (no momentum), 1 (momentum) or 2 (nesterov), got %d",
                   what, d.form);
        SD_REQUIRE(d.op != SD_NN_LAMB || d.rows >= 1, SD_ERR_INVALID, "%s: lamb needs the block count of sd_lamb_table_build in rows (got %d)", what, d.rows);
        return 0;
    case SD_NN_GRAD_ACCUM: return check_grad_accum(what, M, d.form);
    case SD_NN_BN_FOLD: case SD_NN_HEAD_FWD: case SD_NN_HEAD_BWD: return 0;
    }
    SD_REQUIRE(false, SD_ERR_INVALID, "%s: unknown op %d", what, d.op);
    return 0;
}

const char* sd_nn_kernel_names(const sd_nn_call_desc* d) {
    static thread_local char line[1024];
    static const sd_nn_call_desc none = {-1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!d) d = &none;
    Names out{line, sizeof(line), 0};
    line[0] = 0;
    char name[128];
#define NAME(...) (snprintf(name, sizeof(name), __VA_ARGS__), name)
    // a stand-in for pointer k of the op's kernel choice: only its alignment is ever looked at
    const auto ptr = [&](int k) { return reinterpret_cast<const void*>((uintptr_t)((d->flags >> k & 1u) ? 0x1000 : 0x1001)); };
    const int op = d->op, C = d->C, Co = d->Co, Ho = pool_out(d->H), Wo = pool_out(d->W);
    const bool bf = d->form != 0, sums = (d->flags & SD_NN_SUMS) != 0, map_op = op >= SD_NN_MAXPOOL_FWD && op <= SD_NN_UPSAMPLE_BWD;
    const bool head = op == SD_NN_HEAD_FWD || op == SD_NN_HEAD_BWD, wide_head = head && Co > HEAD_NARROW_MAX_CO;
    const char *T = bf ? "unsigned short" : "float", *DT = d->form == 2 ? "unsigned short" : "float";
    const int64_t M = map_op ? (int64_t)d->B * d->H * d->W : head ? (int64_t)d->B * d->H : d->M;
    const bool quad = stem_bwd_quad(d->H, d->W), stem = op >= SD_NN_STEM_BWD && op <= SD_NN_STEM_BWD_APPLY;
    if (check_desc("sd_nn_kernel_names", *d, M)) {
        snprintf(line, sizeof(line), "refused: %s", sd_last_error());
        return line;
    }
    const ColReducePlan p = plan_col_reduce(M, C, stem ? ROWS_STEM_TAIL : ROWS_BN);
    switch (op) {
    case SD_NN_BN_TRAIN_STATS: case SD_NN_COL_SUM:
        out.reduce(NAME("k_col_reduce<%d, %s>", op == SD_NN_COL_SUM ? 2 : 0, T), p.nb, p.fold, op == SD_NN_COL_SUM ? 2 : 0, sums, C);
        out.plan(p);
        break;
    case SD_NN_BN_FINALIZE_STATS: case SD_NN_BN_BWD_FINALIZE: {
        const FoldPlan f = plan_fold(d->rows, C, (d->flags & SD_NN_SCRATCH) != 0);
        out.reduce(nullptr, 0, f, op == SD_NN_BN_BWD_FINALIZE, sums, C);
        out.put(" | slab=%d rows=%d", f.slab, f.rows);
        break;
    }
    case SD_NN_BN_STATS_FROM_SUMS: out.add("k_bn_stats_from_sums", chan_launch(C, 256)); break;
    case SD_NN_BN_BWD_MEANS_FROM_SUMS: out.add("k_bn_bwd_means_from_sums", chan_launch(C, 256)); break;
    case SD_NN_BN_FOLD: out.add("k_bn_fold", chan_launch(C, 256)); break;
    case SD_NN_BN_APPLY:
    {
        const bool wide = bf && bn_apply_wide(C, ptr(0), ptr(1), ptr(2));
        out.add(wide ? "k_bn_apply_bf16x8" : NAME("k_bn_apply<%s>", T), bn_ew_launch(wide, M, C));
        break;
    }
    case SD_NN_BN_BWD: case SD_NN_BN_BWD_REDUCE: case SD_NN_BN_BWD_APPLY: {
        const bool reduce_only = op == SD_NN_BN_BWD_REDUCE;
        const bool wide = bf && bn_bwd_wide(C, d->relu, ptr(0), ptr(1), reduce_only ? nullptr : ptr(2), reduce_only ? nullptr : ptr(3));
        if (op != SD_NN_BN_BWD_APPLY) out.reduce(wide ? "k_col_reduce_bwd_bf16x8" : NAME("k_col_reduce<1, %s>", T), p.nb, p.fold, 1, sums, C);
        if (!reduce_only) out.add(wide ? "k_bn_bwd_apply_bf16x8" : NAME("k_bn_bwd_apply<%s>", T), bn_ew_launch(wide, M, C));
        if (op != SD_NN_BN_BWD_APPLY) out.plan(p);
        break;
    }
    case SD_NN_BN_FROZEN_BWD: {
        const bool wide = frozen_bwd_wide(bf, C, ptr(0), ptr(1), ptr(2), ptr(3));
        out.add(!wide ? NAME("k_bn_frozen_bwd_ew<%s>", T) : bf ? "k_bn_frozen_bwd_bf16x8" : "k_bn_frozen_bwd_f32x4", frozen_bwd_launch(bf, wide, M, C));
        break;
    }
    case SD_NN_MAXPOOL_FWD: out.add(bf ? "k_maxpool_fwd_bf16" : "k_maxpool_fwd", map_launch(d->B, Ho, Wo, C, bf ? 8 : 4)); break;
    case SD_NN_MAXPOOL_BWD: out.add("k_maxpool_bwd", map_launch(d->B, d->H, d->W, C, 4)); break;
    case SD_NN_BN_RELU_MAXPOOL_FWD: {
        const int elems = bf ? 8 : 4;
        const bool pair = pool_fwd_pair(d->pool_fwd_pair, elems, Wo, C, ptr(0), ptr(1), ptr(2));
        out.add(pair ? NAME("k_bn_relu_maxpool_fwd_pair<%s, %s, %d>", T, T, elems) : NAME("k_bn_relu_maxpool_fwd<%s, %s>", T, T), pool_fwd_launch(pair, elems, d->B, Ho, Wo, C));
        break;
    }
    case SD_NN_STEM_BWD: case SD_NN_STEM_BWD_REDUCE: case SD_NN_STEM_BWD_APPLY:
        if (op != SD_NN_STEM_BWD_APPLY) out.reduce(quad ? NAME("k_pool_bn_bwd_reduce_quad<%s, %s>", T, T) : "k_pool_bn_bwd_reduce", p.nb, p.fold, 1, sums, C);
        if (op != SD_NN_STEM_BWD_REDUCE) out.add(quad ? NAME("k_pool_bn_bwd_apply_quad<%s, %s, %s>", T, T, DT) : "k_pool_bn_bwd_apply", stem_apply_launch(quad, d->B, d->H, d->W, C));
        if (op != SD_NN_STEM_BWD_APPLY) out.plan(p);
        break;
    case SD_NN_UPSAMPLE_BWD: out.add(NAME("k_up2_bwd<%s>", T), map_launch(d->B, d->H, d->W, C, 4)); break;
    case SD_NN_CAST: out.add(bf ? "k_cast_f32" : "k_cast_bf16", ew_launch(M / 4)); break;
    case SD_NN_HEAD_FWD: {
        const HeadLaunch l = plan_head_fwd(bf, M, d->H, C, Co, ptr(0), ptr(1), ptr(2));
        if (wide_head) out.put(bf ? "head_wide_fwd_bf16" : "head_wide_fwd");
        else if (bf) out.add(l.c128 ? (Co <= 16 ? "k_head_fwd_bf16_c128<false>" : "k_head_fwd_bf16_c128<true>") : "k_head_fwd_bf16", l.grid, l.lds);
        else out.add(l.c128 ? "k_head_fwd_f32_c128" : "k_head_fwd", l.grid, l.lds);
        break;
    }
    case SD_NN_HEAD_BWD: {
        const HeadLaunch l = plan_head_wgrad(!bf && head_wgrad_f32_c128(M, d->H, C, Co, ptr(0), ptr(1)), M);
        if (wide_head) out.put("head_wide_wgrad");
        else if (bf) { out.add("k_head_dgrad<unsigned short>", head_dgrad_launch(M, C, Co)); out.add("k_head_wgrad_bf16<8>", l.grid); }
        else out.add(l.c128 ? "k_head_wgrad_f32_c128" : "k_head_wgrad", l.grid, l.lds);
        out.add("k_head_wgrad_fin", head_fin_grid(C, Co));
        if (wide_head) out.put("; head_wide_dgrad");
        else if (!bf) out.add("k_head_dgrad<float>", head_dgrad_launch(M, C, Co));
        out.put(" | ws_bytes=%zu", sd_head_bwd_workspace_bytes(d->B, d->H, C, Co));
        break;
    }
    case SD_NN_ADAM: out.add("k_adam", ew_launch(M / 4)); break;
    case SD_NN_GRAD_SUMSQ:
        out.add("k_grad_sumsq", sumsq_blocks(M));
        out.put(" | ws_bytes=%zu", sd_grad_sumsq_workspace_bytes(M));
        break;
    case SD_NN_OPTIM: {
        const bool decay = d->flags & SD_NN_DECAY, clip = d->flags & SD_NN_CLIP, avg = d->flags & SD_NN_EMA;
        static const char* const tf[2] = {"false", "true"};
        out.add(decay || clip || avg ? NAME("k_optim<%s, %s, %s>", tf[decay], tf[clip], tf[avg]) : "k_adam", ew_launch(M / 4));
        break;
    }
    case SD_NN_OPTIM_GROUPS: {                                                 // the step's two calls: sd_grad_sumsq (with clipping), sd_optim_groups_step
        const bool clip = d->flags & SD_NN_CLIP, avg = d->flags & SD_NN_EMA;
        static const char* const tf[2] = {"false", "true"};
        if (clip) out.add("k_grad_sumsq", sumsq_blocks(M));
        out.add(NAME("k_optim_groups<%s, %s>", tf[clip], tf[avg]), ew_launch(M / 4));
        break;
    }
    case SD_NN_SGD: {                                                          // sd_grad_sumsq (with clipping), sd_sgd_step; form = momentum kind
        const bool clip = d->flags & SD_NN_CLIP, avg = d->flags & SD_NN_EMA;
        static const char* const tf[2] = {"false", "true"};
        if (clip) out.add("k_grad_sumsq", sumsq_blocks(M));
        out.add(NAME("k_sgd<%d, %s, %s>", d->form, tf[clip], tf[avg]), ew_launch(M / 4));
        break;
    }
    case SD_NN_LAMB: {                                                         // sd_grad_sumsq (with clipping), sd_lamb_step's two passes; rows = its nblocks
        const bool clip = d->flags & SD_NN_CLIP, avg = d->flags & SD_NN_EMA;
        static const char* const tf[2] = {"false", "true"};
        if (clip) out.add("k_grad_sumsq", sumsq_blocks(M));
        out.add(NAME("k_lamb_moments<%s>", tf[clip]), d->rows);
        out.add(NAME("k_lamb_apply<%s, %s>", tf[clip], tf[avg]), d->rows);
        out.put(" | ws_bytes=%zu", sd_lamb_workspace_bytes(d->rows));
        break;
    }
    case SD_NN_GRAD_ACCUM:                                                     // n == 0: no launch, an empty answer
        if (M > 0) out.add(bf ? "k_grad_accum<true>" : "k_grad_accum<false>", ew_launch(M / 4));
        break;
    }
#undef NAME
    return line;
}

}  // extern "C"
