// Flip test-time augmentation for gfx950: the mirrored input batch (sd_tta_views) and the merge of the V head outputs into ONE
// suppressed probability map (sd_tta_merge_nms), and the multi-scale merge (sd_tta_scale_merge_nms): the S x V head outputs of S input
// sizes resampled to the base grid, averaged and suppressed in one launch.  No reference counterpart (the reference has no test-time
// augmentation).  The merged value decides which pixels survive the NMS and is compared bit for bit with the library's own primitives
// (sd_clamped_sigmoid, sd_nms5): separately rounded multiplies and adds, resampling coordinates in double -- floating-point contraction
// is OFF in this file.
#pragma clang fp contract(off)
#include "sd_views.h"

namespace sd {

// ---------------------------------------------------------------------------------------------
// Views.  One thread per group of four input pixels of a row (VEC) or per pixel: the input is read ONCE, as contiguous spans, and every
// view is written from registers.  A mirrored row leaves as one contiguous span too -- lane i of a wave writes the group W4-1-i with
// its four components swapped, so a wave's 1 KiB of a row stays 1 KiB of the mirrored row, only in descending lane order.
// ---------------------------------------------------------------------------------------------
template <int V, bool VEC>
__global__ __launch_bounds__(256) void k_tta_views(const float* __restrict__ x, float* __restrict__ out, int64_t planes, int H, int W,
                                                   ViewFlips vf) {
    const int wg = VEC ? W >> 2 : W;                                   // groups per row
    const int64_t n = planes * H * wg;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int64_t row = i / wg;
    const int g = (int)(i - row * wg);
    const int64_t plane = row / H;
    const int y = (int)(row - plane * H);
    if (VEC) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const bool hf = vf.f[k] & 1;
            const int dy = (vf.f[k] & 2) ? H - 1 - y : y;
            const int dg = hf ? wg - 1 - g : g;
            reinterpret_cast<float4*>(out)[(((int64_t)k * planes + plane) * H + dy) * wg + dg] =
                hf ? reversed(v) : v;
        }
    } else {
        const float v = x[i];
#pragma unroll
        for (int k = 0; k < V; ++k) {
            const int dy = (vf.f[k] & 2) ? H - 1 - y : y;
            const int dg = (vf.f[k] & 1) ? W - 1 - g : g;
            out[(((int64_t)k * planes + plane) * H + dy) * W + dg] = v;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Merge + NMS.  One 256-thread block per 64x16 output tile of one merged map (the tile of sd_nms5).  The tile and its 2-pixel halo are
// staged in LDS as m = (s_0 + s_1 [+ s_2 + s_3]) * (1/V), s_v = clamped_sigmoid(view v's logit at the mirrored coordinate); the 5-max
// is separable (row pass into a second LDS array, column pass in registers); out = (m == max5x5(m)) ? m : 0 with -inf padding.
// Every view's logits are read once (+ the halo re-reads, served by L2), the output is written once.  The tile constants, the staging
// (plain_load_* / plain_sum_*; VEC: 16-byte loads, w % 4 == 0 and 16-byte aligned planes) and the NMS tail (nms5_tile_store) are
// sd_views.h's, shared with k_d4_merge_nms and k_tile_merge_nms.
// ---------------------------------------------------------------------------------------------

template <int V, bool VEC>
__global__ __launch_bounds__(256) void k_tta_merge_nms(const float* __restrict__ hm, int64_t sb, int64_t sc, int B, int C, int h, int w,
                                                       int tiles_x, ViewFlips vf, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float S[LH][LWV];
    __shared__ __attribute__((aligned(16))) float Hm[LH][TW];
    constexpr float inv = 1.0f / V;                                    // 0.5, 0.25: exact
    const int tid = threadIdx.x;
    const int b = blockIdx.z, c = blockIdx.y;
    const int tx0 = (blockIdx.x % tiles_x) * TW;
    const int ty0 = (blockIdx.x / tiles_x) * TH;
    const float* plane[V];
#pragma unroll
    for (int v = 0; v < V; ++v) plane[v] = hm + ((int64_t)v * B + b) * sb + (int64_t)c * sc;

    // all loads of the thread are issued before the first use; cells outside the map read element 0 and become -inf
    if (VEC) {
        float4 ld[NLDV][V];
        plain_load_vec(ld, plane, vf, tid, ty0, tx0, h, w);
#pragma unroll
        for (int j = 0; j < NLDV; ++j) {
            const TileCell t = plain_cell_vec(tid + j * 256, ty0, tx0, h, w);
            float4 m = plain_sum_vec(ld[j], vf);
            m.x = m.x * inv; m.y = m.y * inv; m.z = m.z * inv; m.w = m.w * inv;
            if (!t.ok) m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            if (t.in) *reinterpret_cast<float4*>(&S[t.r][t.c]) = m;
        }
    } else {
        float ld[NLDS][V];
        plain_load_scalar(ld, plane, vf, tid, ty0, tx0, h, w);
#pragma unroll
        for (int j = 0; j < NLDS; ++j) {
            const TileCell t = plain_cell_scalar(tid + j * 256, ty0, tx0, h, w);
            const float m = plain_sum_scalar(ld[j]) * inv;
            if (t.in) S[t.r][t.c] = t.ok ? m : -INFINITY;
        }
    }
    __syncthreads();
    nms5_tile_store(S, Hm, tid, ty0, tx0, h, w, out + ((int64_t)b * C + c) * h * w, VEC);
}

// ---------------------------------------------------------------------------------------------
// Scale merge + NMS (multi-scale test-time augmentation).  The block and its tile are those of k_tta_merge_nms; the S x V head tensors
// have sizes of their own and are resampled to the base grid (bilinear, half-pixel centres: F.interpolate's align_corners=False).
// Per scale the block computes the 68 + 20 per-axis entries (x0, x1, wx0, wx1) of its tile + halo once, in double (scale_axis); per
// (scale, view) it stages clamped_sigmoid of the source footprint of the tile in LDS ONCE per source cell (F, in MEMORY coordinates:
// a mirrored view is mirrored when F is indexed, so the staged span of a row is contiguous either way) and every base cell adds its
// interpolated sample to a register accumulator -- scale-major, view-minor, each product and add rounded separately.  The mean then
// goes through the separable 5-max of k_tta_merge_nms.
//   footprint: hs <= 2h, ws <= 2w (checked on the host) bound it to 138 x 42 source cells for the 68 x 20 base cells; the 16-byte
//   variant widens a row's span to whole aligned groups (<= 36 groups = FW columns).  The staging loops are clamped to F's extent.
//   16-byte loads per scale when ws % 4 == 0 and the planes / strides are 16-byte aligned (a group is then entirely inside a row),
//   4-byte loads otherwise.
// ---------------------------------------------------------------------------------------------
constexpr int MAX_SCALES = 5;
constexpr int FH = 42, FW = 144;

struct ScaleArgs {
    const float* hm[MAX_SCALES];
    int64_t sb[MAX_SCALES], sc[MAX_SCALES];
    double rx[MAX_SCALES], ry[MAX_SCALES];          // (double)ws / (double)w, (double)hs / (double)h
    int hs[MAX_SCALES], ws[MAX_SCALES];
    unsigned char vec[MAX_SCALES];
};

// one axis entry of the resampling: source cells i0, i1 and their weights for base cell `i` (n_in source cells, ratio = n_in / n_out)
__device__ __forceinline__ void scale_axis(int i, double ratio, int n_in, int* i0, int* i1, float* w0, float* w1) {
    const double t = ((double)i + 0.5) * ratio;
    const double s = fmax(t - 0.5, 0.0);
    const int a = min((int)floor(s), n_in - 1);
    const double lam = s - (double)a;
    *i0 = a;
    *i1 = min(a + 1, n_in - 1);
    *w1 = (float)lam;
    *w0 = (float)(1.0 - lam);
}

template <int V>
__global__ __launch_bounds__(256) void k_tta_scale_merge_nms(ScaleArgs sa, int S, float inv, int B, int C, int h, int w, int tiles_x,
                                                             ViewFlips vf, int out_vec, float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float F[FH][FW];
    __shared__ __attribute__((aligned(16))) float Sm[LH][LWV];
    __shared__ __attribute__((aligned(16))) float Hm[LH][TW];
    __shared__ int X0[LWS], X1[LWS], Y0[LH], Y1[LH];
    __shared__ float WX0[LWS], WX1[LWS], WY0[LH], WY1[LH];
    constexpr int NC = LH * LWS;                                       // 1360 base cells (tile + halo)
    constexpr int NA = (NC + 255) / 256;
    const int tid = threadIdx.x;
    const int b = blockIdx.z, c = blockIdx.y;
    const int tx0 = (blockIdx.x % tiles_x) * TW;
    const int ty0 = (blockIdx.x / tiles_x) * TH;
    float acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[j] = 0.0f;

    for (int s = 0; s < S; ++s) {
        const int hs = sa.hs[s], ws = sa.ws[s];
        // axis tables of this scale; cells of the halo outside the map take the entry of the nearest cell inside (never sampled, but the
        // first and the last entry bound the footprint)
        if (tid < LWS) {
            scale_axis(min(max(tx0 + tid - HALO, 0), w - 1), sa.rx[s], ws, &X0[tid], &X1[tid], &WX0[tid], &WX1[tid]);
        } else if (tid < LWS + LH) {
            const int r = tid - LWS;
            scale_axis(min(max(ty0 + r - HALO, 0), h - 1), sa.ry[s], hs, &Y0[r], &Y1[r], &WY0[r], &WY1[r]);
        }
        __syncthreads();
        const int xa = X0[0], xb = X1[LWS - 1], ya = Y0[0], yb = Y1[LH - 1];      // the footprint in view coordinates (monotone tables)
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const bool hf = vf.f[v] & 1, vfl = vf.f[v] & 2;
            const float* plane = sa.hm[s] + ((int64_t)v * B + b) * sa.sb[s] + (int64_t)c * sa.sc[s];
            const int mya = vfl ? hs - 1 - yb : ya;                    // the footprint in memory coordinates
            const int rows = min(yb - ya + 1, FH);
            int mxa = hf ? ws - 1 - xb : xa;
            if (sa.vec[s]) {
                mxa &= ~3;
                const int mxb = hf ? ws - 1 - xa : xb;
                const int groups = min((mxb >> 2) - (mxa >> 2) + 1, FW / 4);
                const int n = rows * groups;
                for (int i = tid; i < n; i += 256) {
                    const int r = i / groups, q = i - r * groups;
                    const float4 t = *reinterpret_cast<const float4*>(plane + (int64_t)(mya + r) * ws + mxa + 4 * q);
                    *reinterpret_cast<float4*>(&F[r][4 * q]) =
                        make_float4(clamped_sigmoid(t.x), clamped_sigmoid(t.y), clamped_sigmoid(t.z), clamped_sigmoid(t.w));
                }
            } else {
                const int cols = min(xb - xa + 1, FW);
                const int n = rows * cols;
                for (int i = tid; i < n; i += 256) {
                    const int r = i / cols, q = i - r * cols;
                    F[r][q] = clamped_sigmoid(plane[(int64_t)(mya + r) * ws + mxa + q]);
                }
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                const int i = tid + j * 256;
                const int r = i / LWS, cc = i - r * LWS;
                const int y = ty0 + r - HALO, x = tx0 + cc - HALO;
                if (i < NC && y >= 0 && y < h && x >= 0 && x < w) {
                    const int fx0 = (hf ? ws - 1 - X0[cc] : X0[cc]) - mxa, fx1 = (hf ? ws - 1 - X1[cc] : X1[cc]) - mxa;
                    const int fy0 = (vfl ? hs - 1 - Y0[r] : Y0[r]) - mya, fy1 = (vfl ? hs - 1 - Y1[r] : Y1[r]) - mya;
                    const float wx0 = WX0[cc], wx1 = WX1[cc], wy0 = WY0[r], wy1 = WY1[r];
                    const float top = wx0 * F[fy0][fx0] + wx1 * F[fy0][fx1];
                    const float bot = wx0 * F[fy1][fx0] + wx1 * F[fy1][fx1];
                    const float rv = wy0 * top + wy1 * bot;
                    acc[j] = acc[j] + rv;                              // 0 + r_{0,0} is r_{0,0}
                }
            }
            __syncthreads();                                           // F and the tables are rewritten by the next view / scale
        }
    }
#pragma unroll
    for (int j = 0; j < NA; ++j) {
        const int i = tid + j * 256;
        const int r = i / LWS, cc = i - r * LWS;
        const int y = ty0 + r - HALO, x = tx0 + cc - HALO;
        if (i < NC) Sm[r][cc + OFF - HALO] = (y >= 0 && y < h && x >= 0 && x < w) ? acc[j] * inv : -INFINITY;
    }
    __syncthreads();
    nms5_tile_store(Sm, Hm, tid, ty0, tx0, h, w, out + ((int64_t)b * C + c) * h * w, out_vec != 0);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static void launch_merge_nms(int V, bool vec, dim3 grid, hipStream_t st, const float* hm, int64_t sb, int64_t sc, int B, int C, int h, int w,
                             int tiles_x, ViewFlips vf, float* out) {
    with_views<true>(V, [&](auto v) {
        with_flag(vec, [&](auto vc) {
            hipLaunchKernelGGL((k_tta_merge_nms<decltype(v)::value, decltype(vc)::value>), grid, dim3(256), 0, st, hm, sb, sc, B, C, h, w,
                               tiles_x, vf, out);
        });
    });
}

}  // namespace sd

using namespace sd;

extern "C" {

int sd_tta_views(const float* x, float* out, int B, int H, int W, int V, const unsigned char* view_flips, sd_stream_t stream) {
    SD_REQUIRE(x != nullptr && out != nullptr, SD_ERR_INVALID, "sd_tta_views: null pointer");
    SD_REQUIRE(B > 0 && H > 0 && W > 0, SD_ERR_INVALID, "sd_tta_views: bad shape (%d,3,%d,%d)", B, H, W);
    ViewFlips vf;
    if (int e = check_views("sd_tta_views", V, view_flips, &vf)) return e;
    const int64_t planes = (int64_t)B * 3;
    const bool vec = (W % 4 == 0) && aligned16(x) && aligned16(out);
    const int64_t blocks = (planes * H * (vec ? W / 4 : W) + 255) / 256;
    SD_REQUIRE(blocks < (1ll << 31), SD_ERR_INVALID, "sd_tta_views: %lld blocks exceed the grid", (long long)blocks);
    const dim3 grid((unsigned)blocks), block(256);
    const hipStream_t st = (hipStream_t)stream;
    with_views<false>(V, [&](auto v) {
        with_flag(vec, [&](auto vc) {
            hipLaunchKernelGGL((k_tta_views<decltype(v)::value, decltype(vc)::value>), grid, block, 0, st, x, out, planes, H, W, vf);
        });
    });
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_tta_merge_nms(const float* hm, int64_t sb, int64_t sc, float* out, int B, int C, int h, int w, int V,
                     const unsigned char* view_flips, sd_stream_t stream) {
    const char* fn = "sd_tta_merge_nms";
    SD_REQUIRE(hm != nullptr && out != nullptr, SD_ERR_INVALID, "%s: null pointer", fn);
    ViewFlips vf;
    if (int e = check_merge_args(fn, B, C, h, w, V, view_flips, &vf, false)) return e;
    SD_REQUIRE(sc >= (int64_t)h * w && sb >= (int64_t)h * w, SD_ERR_INVALID, "%s: bad strides sb=%lld sc=%lld", fn, (long long)sb, (long long)sc);
    SD_REQUIRE(C <= 65535 && B <= 65535, SD_ERR_INVALID, "%s: B=%d, C=%d exceed the grid (65535)", fn, B, C);
    const int tiles_x = cdiv(w, TW), tiles_y = cdiv(h, TH);
    const bool vec = (w % 4 == 0) && aligned16(hm) && aligned16(out) && sb % 4 == 0 && sc % 4 == 0;
    const dim3 grid(tiles_x * tiles_y, C, B);
    const hipStream_t st = (hipStream_t)stream;
    launch_merge_nms(V, vec, grid, st, hm, sb, sc, B, C, h, w, tiles_x, vf, out);
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_tta_scale_merge_nms(const float* const* hm_host, const int64_t* sb_host, const int64_t* sc_host, const int* hs_host,
                           const int* ws_host, float* out, int B, int C, int h, int w, int S, int V,
                           const unsigned char* view_flips_host, sd_stream_t stream) {
    const char* fn = "sd_tta_scale_merge_nms";
    SD_REQUIRE(hm_host != nullptr && sb_host != nullptr && sc_host != nullptr && hs_host != nullptr && ws_host != nullptr && out != nullptr,
               SD_ERR_INVALID, "%s: null pointer", fn);
    SD_REQUIRE(S >= 1 && S <= MAX_SCALES, SD_ERR_INVALID, "%s: S=%d scales (1 .. %d are supported)", fn, S, MAX_SCALES);
    ViewFlips vf;
    if (int e = check_merge_args(fn, B, C, h, w, V, view_flips_host, &vf, true)) return e;
    SD_REQUIRE(C <= 65535 && B <= 65535, SD_ERR_INVALID, "%s: B=%d, C=%d exceed the grid (65535)", fn, B, C);
    ScaleArgs sa{};
    for (int s = 0; s < S; ++s) {
        const int hs = hs_host[s], ws = ws_host[s];
        SD_REQUIRE(hm_host[s] != nullptr, SD_ERR_INVALID, "%s: null pointer (scale %d)", fn, s);
        SD_REQUIRE(hs >= 1 && ws >= 1, SD_ERR_INVALID, "%s: scale %d has an empty map (%d,%d)", fn, s, hs, ws);
        // the bound that fits a tile's source footprint into LDS
        SD_REQUIRE(hs <= 2 * (int64_t)h && ws <= 2 * (int64_t)w, SD_ERR_INVALID,
                   "%s: scale %d map (%d,%d) is more than twice the base grid (%d,%d)", fn, s, hs, ws, h, w);
        SD_REQUIRE(sc_host[s] >= (int64_t)hs * ws && sb_host[s] >= (int64_t)hs * ws, SD_ERR_INVALID,
                   "%s: bad strides sb=%lld sc=%lld (scale %d)", fn, (long long)sb_host[s], (long long)sc_host[s], s);
        sa.hm[s] = hm_host[s];
        sa.sb[s] = sb_host[s];
        sa.sc[s] = sc_host[s];
        sa.hs[s] = hs;
        sa.ws[s] = ws;
        sa.rx[s] = (double)ws / (double)w;
        sa.ry[s] = (double)hs / (double)h;
        sa.vec[s] = (ws % 4 == 0) && aligned16(hm_host[s]) && sb_host[s] % 4 == 0 && sc_host[s] % 4 == 0;
    }
    const int tiles_x = cdiv(w, TW), tiles_y = cdiv(h, TH);
    const bool out_vec = (w % 4 == 0) && aligned16(out);
    const dim3 grid(tiles_x * tiles_y, C, B), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (S == 1 && sa.hs[0] == h && sa.ws[0] == w) {
        // nothing to resample (x0 = x, weights 1 and 0: the same values): the flip merge's kernel, whose sum stays in registers
        launch_merge_nms(V, out_vec && sa.vec[0], grid, st, sa.hm[0], sa.sb[0], sa.sc[0], B, C, h, w, tiles_x, vf, out);
        SD_LAUNCH_CHECK();
        return 0;
    }
    const float inv = (float)(1.0 / (double)(S * V));
    with_views<true>(V, [&](auto v) {
        hipLaunchKernelGGL((k_tta_scale_merge_nms<decltype(v)::value>), grid, block, 0, st, sa, S, inv, B, C, h, w, tiles_x, vf, (int)out_vec, out);
    });
    SD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
