// Head for wide label sets: the 1x1 conv C -> Co with 33 <= Co <= SD_HEAD_MAX_CO (256) output channels, C in {64, 128, 256}
// (network.py:22-29,57 with M + N up to 252).  At these widths the head stops being an HBM stream: at bs = 64, 512 x 512 and
// Co = 256 every pass is a 1M x 128 x 256 GEMM over pixels, bound by the fp32 MFMA.  All four kernels are GEMMs on
// v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 sums) or, for the bf16 activation, v_mfma_f32_32x32x16_bf16 with the fp32 weights
// split into two bf16 terms.  Every wave works on its own: one operand tile (32 rows of the weights) sits in its registers for the
// whole launch, the other is streamed from global memory one 32-pixel tile at a time, and the 32 x 32 result goes straight from the
// accumulator to memory.  No LDS, no block barrier.
//
//   C/D map of the 32x32 MFMAs: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
//   f32 A/B operands: lane (r = lane & 31, h = lane >> 5) holds A[r][k = h] / B[k = h][r] of each step.  The k order is permuted so that
//   a lane's four consecutive steps read four consecutive floats (one 16-byte load): step 4 j + s of lane half h is element 8 j + 4 h + s.
//
// The narrow head (Co <= 32) keeps its kernels in sd_nn.hip; the entry points there hand Co > 32 to the functions at the end of this file.
#include "sd_common.h"
#include "sd_mfma.h"
#include <algorithm>

namespace sd {

// row of the 32x32 accumulator held in register `reg` of lane half `h`
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// ------------------------------------------------------------------------------------------
// fp32 forward: y[b][co][pix] = bias[co] + sum_c w[co][c] x[p][c].  A = 32 output channels of w (C / 2 floats per lane, in registers),
// B = 32 pixels of x (NHWC: lane (r, h) reads pixel r, 16 bytes per load), D = 32 channels x 32 pixels: each accumulator register is
// 32 consecutive pixels of one output plane (128-byte stores).  Wave g serves channel tile g % NT and every nstreams-th pixel tile from
// g / NT: the NT waves of a pixel tile are neighbours, so x comes from HBM once and from L2 for the other channel tiles.
// ------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void k_headw_fwd_f32(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int P, int HW, int Co, int NT, int nstreams) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (g >= NT * nstreams) return;
    const int t = g % NT, q = g / NT;
    const int r = lane & 31, h = lane >> 5;
    const int co = t * 32 + r;
    f32x4 a[C / 8];
#pragma unroll
    for (int j = 0; j < C / 8; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) a[j][s] = co < Co ? w[co * C + 8 * j + 4 * h + s] : 0.f;
    float bv[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int c = t * 32 + acc_row(reg, h);
        bv[reg] = c < Co ? bias[c] : 0.f;
    }
    const int ntiles = (P + 31) >> 5;
    for (int tile = q; tile < ntiles; tile += nstreams) {
        const int p = tile * 32 + r;
        const bool in = p < P;
        const float* xp = x + (int64_t)(in ? p : P - 1) * C + 4 * h;          // (a pixel past the end reads the last one; never stored)
        f32x16 acc = {};
#pragma unroll
        for (int j0 = 0; j0 < C / 8; j0 += 8) {
            f32x4 b[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) b[u] = *reinterpret_cast<const f32x4*>(xp + 8 * (j0 + u));
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j0 + u][s], b[u][s], acc, 0, 0, 0);
        }
        if (in) {
            const int b = p / HW, pix = p - b * HW;
            float* yp = y + (int64_t)b * Co * HW + pix;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int c = t * 32 + acc_row(reg, h);
                if (c < Co) yp[(int64_t)c * HW] = acc[reg] + bv[reg];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// bf16 forward: the same tiling on v_mfma_f32_32x32x16_bf16.  x is bf16 NHWC (lane (r, h) of step s holds x[p][16 s + 8 h .. + 7]: one
// 16-byte load), the fp32 weights are split w = hi + lo into two bf16 terms (|w - hi - lo| <= 2^-17 |w|), so x * hi + x * lo summed in
// fp32 equals the fp32 product to fp32 rounding -- the split k_head_fwd_bf16_c128 uses.  Two MFMAs per step into one accumulator.
// ------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void k_headw_fwd_bf16(const uint16_t* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                         float* __restrict__ y, int P, int HW, int Co, int NT, int nstreams) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (g >= NT * nstreams) return;
    const int t = g % NT, q = g / NT;
    const int r = lane & 31, h = lane >> 5;
    const int co = t * 32 + r;
    bf16x8 ah[C / 16], al[C / 16];
#pragma unroll
    for (int s = 0; s < C / 16; ++s) {
        uint16_t hi[8], lo[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float wv = co < Co ? w[co * C + 16 * s + 8 * h + k] : 0.f;
            hi[k] = f2bf(wv);
            lo[k] = f2bf(wv - bf2f(hi[k]));
        }
        ah[s] = __builtin_bit_cast(bf16x8, hi);
        al[s] = __builtin_bit_cast(bf16x8, lo);
    }
    float bv[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int c = t * 32 + acc_row(reg, h);
        bv[reg] = c < Co ? bias[c] : 0.f;
    }
    constexpr int CH = C / 16 < 8 ? C / 16 : 8;                                // steps per batch of loads
    const int ntiles = (P + 31) >> 5;
    for (int tile = q; tile < ntiles; tile += nstreams) {
        const int p = tile * 32 + r;
        const bool in = p < P;
        const uint16_t* xp = x + (int64_t)(in ? p : P - 1) * C + 8 * h;
        f32x16 acc = {};
#pragma unroll
        for (int s0 = 0; s0 < C / 16; s0 += CH) {
            bf16x8 b[CH];
#pragma unroll
            for (int u = 0; u < CH; ++u) b[u] = *reinterpret_cast<const bf16x8*>(xp + 16 * (s0 + u));
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s0 + u], b[u], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s0 + u], b[u], acc, 0, 0, 0);
            }
        }
        if (in) {
            const int b = p / HW, pix = p - b * HW;
            float* yp = y + (int64_t)b * Co * HW + pix;
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int c = t * 32 + acc_row(reg, h);
                if (c < Co) yp[(int64_t)c * HW] = acc[reg] + bv[reg];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------
// data gradient: dx[p][c] = sum_co dy[b][co][pix] w[co][c], K = Co (padded to 32 NT with zeros).  Oriented so that the result rows are
// pixels and the columns channels: A = 32 pixels of dy (lane (r, h) reads pixel r of planes 8 j + 4 h + s: 32 consecutive floats of
// a plane per half-wave), B = 32 input channels of w (32 NT / 2 floats per lane, in registers), and each accumulator register is
// 32 consecutive channels of one NHWC pixel row (128-byte stores).  Wave g serves channel tile g % NC of every nstreams-th pixel tile.
// ------------------------------------------------------------------------------------------
template <int NT>
__global__ __launch_bounds__(256) void k_headw_dgrad(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx,
                                                      int P, int HW, int C, int Co, int NC, int nstreams) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    if (g >= NC * nstreams) return;
    const int ct = g % NC, q = g / NC;
    const int r = lane & 31, h = lane >> 5;
    const int c = ct * 32 + r;
    f32x4 bw[NT * 4];
#pragma unroll
    for (int j = 0; j < NT * 4; ++j)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int co = 8 * j + 4 * h + s;
            bw[j][s] = co < Co ? w[co * C + c] : 0.f;
        }
    const int ntiles = (P + 31) >> 5;
    for (int tile = q; tile < ntiles; tile += nstreams) {
        const int p = tile * 32 + r;
        const int pp = p < P ? p : P - 1;
        const int b = pp / HW, pix = pp - b * HW;
        const float* dp = dy + (int64_t)b * Co * HW + pix;
        f32x16 acc = {};
#pragma unroll
        for (int j0 = 0; j0 < NT * 4; j0 += 4) {
            f32x4 a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int co = 8 * (j0 + u) + 4 * h + s;
                    a[u][s] = co < Co ? dp[(int64_t)co * HW] : 0.f;
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][s], bw[j0 + u][s], acc, 0, 0, 0);
        }
        float* xp = dx + (int64_t)tile * 32 * C + c;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int pr = acc_row(reg, h);
            if (tile * 32 + pr < P) xp[(int64_t)pr * C] = acc[reg];
        }
    }
}

// ------------------------------------------------------------------------------------------
// weight / bias gradient partials: dw[co][c] = sum_p dy[b][co][pix] x[p][c] over a fixed pixel range [rr span, (rr + 1) span) per
// partial row rr (K = pixels).  A = 32 planes of dy (lane (r, h) of a group of 8 pixels holds pixels 4 h .. 4 h + 3 of plane r: one
// 16-byte load when HW % 4 == 0), B = 32 channels of x, D = 32 x 32 of the partial row.  Waves of channel-tile column 0 also sum their
// dy values: the bias gradient.  Wave g: output tile g % (NT NC), partial row g / (NT NC); the tiles of one pixel range are neighbours.
// Fixed tiling and order: the same call gives the same bits.
// ------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void k_headw_wgrad(const float* __restrict__ dy, const float* __restrict__ x, float* __restrict__ partial,
                                                      int P, int HW, int C, int Co, int NT, int NC, int rows, int span) {
    const int lane = threadIdx.x & 63;
    const int g = blockIdx.x * 4 + (int)(threadIdx.x >> 6);
    const int tiles = NT * NC;
    if (g >= tiles * rows) return;
    const int tl = g % tiles, rr = g / tiles;
    const int t = tl / NC, ct = tl - t * NC;
    const int r = lane & 31, h = lane >> 5;
    const int co = t * 32 + r, c = ct * 32 + r;
    const bool co_in = co < Co;
    const int coc = co_in ? co : Co - 1;
    const int p_begin = rr * span, p_end = min(P, p_begin + span);
    f32x16 acc = {};
    float bsum = 0.f;
    for (int p0 = p_begin; p0 < p_end; p0 += 32) {
        f32x4 a[4], bx[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int pg = p0 + 8 * u + 4 * h;                                 // this lane's four pixels: pg .. pg + 3
            if constexpr (VEC) {
                // HW % 4 == 0: the four pixels lie in one image and p_end % 4 == 0, so they are all in range or all out
                a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (pg < p_end) {
                    const int b = pg / HW, pix = pg - b * HW;
                    const f32x4 v = *reinterpret_cast<const f32x4*>(dy + ((int64_t)b * Co + coc) * HW + pix);
                    if (co_in) a[u] = v;
                }
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int p = pg + s;
                    float v = 0.f;
                    if (p < p_end && co_in) {
                        const int b = p / HW, pix = p - b * HW;
                        v = dy[((int64_t)b * Co + co) * HW + pix];
                    }
                    a[u][s] = v;
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const int p = pg + s;
                bx[u][s] = p < p_end ? x[(int64_t)p * C + c] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][s], bx[u][s], acc, 0, 0, 0);
        if (ct == 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) bsum += (a[u][0] + a[u][1]) + (a[u][2] + a[u][3]);
        }
    }
    const int n = Co * C + Co;
    float* dst = partial + (int64_t)rr * n;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int cr = t * 32 + acc_row(reg, h);
        if (cr < Co) dst[cr * C + c] = acc[reg];
    }
    if (ct == 0) {
        const float tot = bsum + __shfl_xor(bsum, 32, 64);                    // (the two lane halves: a + b == b + a)
        if (h == 0 && co_in) dst[Co * C + co] = tot;
    }
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
namespace {

bool wide_depth_ok(int C) { return C == 64 || C == 128 || C == 256; }

// blocks of 256 threads of `kernel` resident on the current device at once (the wave streams of the forward / data-gradient
// kernels are sized to it so that every stream runs from the start; the result never changes what is computed)
template <typename K>
int resident_blocks(K kernel) {
    int dev = 0, cus = 0, per_cu = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), 256, 0) != hipSuccess || per_cu < 1) per_cu = 1;
    return cus * per_cu;
}

// streams of pixel tiles for a launch of `tiles_per_px` waves per pixel tile: all resident, at most one per pixel tile
int wave_streams(int resident, int tiles_per_px, int P) {
    return std::max(1, std::min(resident * 4 / tiles_per_px, cdiv(P, 32)));
}

// partial rows of the weight gradient: about 4096 waves in all, at least 256 pixels (a multiple of 32) per row.  Depends on the
// shape only, so that repeated calls reduce in the same order.
void wgrad_rows(int64_t P, int C, int Co, int& rows, int& span) {
    const int tiles = std::max(1, cdiv(Co, 32) * (C / 32));
    const int want = std::max(1, cdiv(4096, tiles));
    span = std::max(256, cdiv(cdiv(P, want), 32) * 32);
    rows = cdiv(P, span);
}

}  // namespace

int head_wide_check(const char* fn, int64_t P, int C, int Co) {
    SD_REQUIRE(Co > 0 && Co <= SD_HEAD_MAX_CO && wide_depth_ok(C), SD_ERR_INVALID, "%s: needs C in {64, 128, 256} for %d < Co <= %d (got C = %d, Co = %d)",
               fn, HEAD_NARROW_MAX_CO, SD_HEAD_MAX_CO, C, Co);
    SD_REQUIRE(P < (1ll << 31), SD_ERR_INVALID, "%s: B * HW must be < 2^31 for Co > %d", fn, HEAD_NARROW_MAX_CO);
    return 0;
}

int head_wide_fwd(const float* x, const float* w, const float* bias, float* y, int B, int HW, int C, int Co, hipStream_t st) {
    const int64_t P = (int64_t)B * HW;
    if (int e = head_wide_check("sd_head_fwd", P, C, Co)) return e;
    SD_REQUIRE(aligned16(x), SD_ERR_ALIGN, "sd_head_fwd: x must be 16-byte aligned for Co > %d", HEAD_NARROW_MAX_CO);
    const int NT = cdiv(Co, 32);
#define HW_FWD(C_)                                                                                                              \
    {                                                                                                                           \
        static const int res = resident_blocks(k_headw_fwd_f32<C_>);                                                             \
        const int ns = wave_streams(res, NT, (int)P);                                                                           \
        hipLaunchKernelGGL(k_headw_fwd_f32<C_>, dim3(cdiv((int64_t)NT * ns, 4)), dim3(256), 0, st, x, w, bias, y, (int)P, HW, Co, NT, ns); \
    }
    if (C == 64) HW_FWD(64) else if (C == 128) HW_FWD(128) else HW_FWD(256)
#undef HW_FWD
    SD_LAUNCH_CHECK();
    return 0;
}

int head_wide_fwd_bf16(const void* x, const float* w, const float* bias, float* y, int B, int HW, int C, int Co, hipStream_t st) {
    const int64_t P = (int64_t)B * HW;
    if (int e = head_wide_check("sd_head_fwd_bf16", P, C, Co)) return e;
    SD_REQUIRE(aligned16(x), SD_ERR_ALIGN, "sd_head_fwd_bf16: x must be 16-byte aligned for Co > %d", HEAD_NARROW_MAX_CO);
    const int NT = cdiv(Co, 32);
    const uint16_t* xb = (const uint16_t*)x;
#define HW_FWD(C_)                                                                                                              \
    {                                                                                                                           \
        static const int res = resident_blocks(k_headw_fwd_bf16<C_>);                                                            \
        const int ns = wave_streams(res, NT, (int)P);                                                                           \
        hipLaunchKernelGGL(k_headw_fwd_bf16<C_>, dim3(cdiv((int64_t)NT * ns, 4)), dim3(256), 0, st, xb, w, bias, y, (int)P, HW, Co, NT, ns); \
    }
    if (C == 64) HW_FWD(64) else if (C == 128) HW_FWD(128) else HW_FWD(256)
#undef HW_FWD
    SD_LAUNCH_CHECK();
    return 0;
}

size_t head_wide_bwd_workspace_bytes(int64_t P, int C, int Co) {
    int rows = 0, span = 0;
    wgrad_rows(P, C, Co, rows, span);
    return align_up((size_t)rows * ((size_t)Co * C + Co) * sizeof(float), 256);
}

int head_wide_wgrad(const float* dy, const float* x, float* partial, int B, int HW, int C, int Co, hipStream_t st, int& rows) {
    const int64_t P = (int64_t)B * HW;
    int span = 0;
    wgrad_rows(P, C, Co, rows, span);
    const int NT = cdiv(Co, 32), NC = C / 32;
    const int blocks = cdiv((int64_t)NT * NC * rows, 4);
    if (HW % 4 == 0 && aligned16(dy))
        hipLaunchKernelGGL(k_headw_wgrad<true>, dim3(blocks), dim3(256), 0, st, dy, x, partial, (int)P, HW, C, Co, NT, NC, rows, span);
    else
        hipLaunchKernelGGL(k_headw_wgrad<false>, dim3(blocks), dim3(256), 0, st, dy, x, partial, (int)P, HW, C, Co, NT, NC, rows, span);
    SD_LAUNCH_CHECK();
    return 0;
}

int head_wide_dgrad(const float* dy, const float* w, float* dx, int B, int HW, int C, int Co, hipStream_t st) {
    const int64_t P = (int64_t)B * HW;
    const int NT = cdiv(Co, 32), NC = C / 32;
#define HW_DG(NT_)                                                                                                              \
    case NT_: {                                                                                                                 \
        static const int res = resident_blocks(k_headw_dgrad<NT_>);                                                             \
        const int ns = wave_streams(res, NC, (int)P);                                                                           \
        hipLaunchKernelGGL(k_headw_dgrad<NT_>, dim3(cdiv((int64_t)NC * ns, 4)), dim3(256), 0, st, dy, w, dx, (int)P, HW, C, Co, NC, ns); \
        break;                                                                                                                  \
    }
    switch (NT) {
        HW_DG(2) HW_DG(3) HW_DG(4) HW_DG(5) HW_DG(6) HW_DG(7) HW_DG(8)
        default: SD_REQUIRE(false, SD_ERR_INVALID, "sd_head_bwd: Co = %d out of range", Co);
    }
#undef HW_DG
    SD_LAUNCH_CHECK();
    return 0;
}

}  // namespace sd
