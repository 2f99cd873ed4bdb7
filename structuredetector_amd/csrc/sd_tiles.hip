// Tiled inference for gfx950: the overlapping network-input crops of a large canvas (sd_tile_views) and the stitch of the Ty x Tx tile
// head outputs into ONE suppressed probability map on the canvas grid, with the owner tile's regression channels beside it
// (sd_tile_merge_nms).  No reference counterpart (the reference resizes the whole image to one network input).  The blended value
// decides which cells survive the NMS and is compared bit for bit with the library's own primitives (sd_clamped_sigmoid, sd_nms5):
// separately rounded multiplies and adds, ramp weights in double -- floating-point contraction is OFF in this file.
#pragma clang fp contract(off)
#include "sd_views.h"

namespace sd {

// ---------------------------------------------------------------------------------------------
// Views.  One thread per group of four pixels of an OUTPUT row (VEC) or per pixel: every tile row is written as one contiguous span and
// read as one contiguous span of the canvas row (the overlap columns are read twice, by the two tiles that share them; L2 serves the
// second read).
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void k_tile_views(const float* __restrict__ canvas, float* __restrict__ out, int64_t n, int B, int Hc,
                                                    int Wc, int H, int W, int Tx, int O) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int wg = VEC ? W >> 2 : W;                                   // groups per output row
    const int64_t row = i / wg;
    const int g = (int)(i - row * wg);
    const int64_t plane = row / H;                                     // (t*B + b)*3 + c
    const int y = (int)(row - plane * H);
    const int64_t img = plane / 3;
    const int c = (int)(plane - img * 3);
    const int t = (int)(img / B), b = (int)(img - (int64_t)t * B);
    const int tj = t / Tx, ti = t - tj * Tx;
    const int64_t src_row = (((int64_t)b * 3 + c) * Hc + (int64_t)tj * (H - O) + y) * Wc + (int64_t)ti * (W - O);
    if (VEC) reinterpret_cast<float4*>(out)[i] = *reinterpret_cast<const float4*>(canvas + src_row + 4 * g);
    else     out[i] = canvas[src_row + g];
}

// ---------------------------------------------------------------------------------------------
// Merge + NMS.  One 256-thread block per 64x16 CANVAS tile of one merged map (the block of sd_nms5 and sd_tta_merge_nms).  Per block the
// per-axis tables of its 72 staged columns and 20 staged rows are computed once (axis_entry): the upper covering tile, the local
// coordinate in it, whether the tile below it covers the cell as well, the two ramp weights, and the owner tile of the regressions.  At
// most two tiles cover a cell along an axis (2o <= min(h, w)), so a staged cell gathers <= 4 contributions, in ascending tile order
// (row-major), m = sum of (wy * wx) * clamped_sigmoid(logit), every operation rounded separately.  Then the separable 5-max of
// k_tta_merge_nms: out = (m == max5x5(m)) ? m : 0 with -inf padding outside the canvas.
//   VEC: w % 4 == 0, o % 4 == 0 and 16-byte aligned planes.  Tile origins, seams and the canvas width are multiples of 4 then: an aligned
//        group of four canvas columns is an aligned group of every tile that covers it, entirely inside or entirely outside an overlap.
//        The staged span of a row is [tx0-4, tx0+68): 18 groups, each <= 4 16-byte loads (contiguous spans of the source tiles' rows).
//   else: <= 4 4-byte loads per staged cell, [tx0-2, tx0+66).
// LDS column of canvas column x: x - tx0 + OFF (OFF = 4) in both variants; LDS row of canvas row y: y - ty0 + HALO (the tile constants
// and the NMS tail: sd_views.h).
// Blocks with blockIdx.y >= C copy regression plane blockIdx.y - C of the same canvas tile from the owner tiles, unstaged.
// ---------------------------------------------------------------------------------------------
struct AxisEntry {
    int hi;          // the upper covering tile (-1: the cell is outside the canvas)
    int l;           // local coordinate in tile `hi`; tile hi-1 covers the cell at l + (n - o) when `two`
    int two;
    float w_lo, w_hi;
    int own, own_l;  // the owner tile of the regressions and the local coordinate in it
};

// one axis entry for canvas coordinate X: tiles of n cells, overlap o, T tiles, canvas of nc cells
__device__ __forceinline__ AxisEntry axis_entry(int X, int n, int o, int T, int nc) {
    AxisEntry e;
    if (X < 0 || X >= nc) {
        e.hi = -1; e.l = 0; e.two = 0; e.w_lo = 0.0f; e.w_hi = 1.0f; e.own = 0; e.own_l = 0;
        return e;
    }
    const int step = n - o;
    e.hi = min(X / step, T - 1);
    e.l = X - e.hi * step;
    e.two = e.hi > 0 && e.l < o;
    if (e.two) {
        e.w_lo = (float)((double)(o - e.l) / (double)(o + 1));
        e.w_hi = (float)((double)(e.l + 1) / (double)(o + 1));
    } else {
        e.w_lo = 0.0f;
        e.w_hi = 1.0f;
    }
    const bool lower = e.two && (o - e.l) >= (e.l + 1);                // the larger weight owns; a tie goes to the lower tile
    e.own = lower ? e.hi - 1 : e.hi;
    e.own_l = lower ? e.l + step : e.l;
    return e;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_tile_merge_nms(const float* __restrict__ hm, int64_t sb, int64_t sc, int C,
                                                        const float* __restrict__ reg, int64_t r_sb, int64_t r_sc,
                                                        float* __restrict__ out_hm, float* __restrict__ out_reg, int B, int h, int w,
                                                        int Ty, int Tx, int o, int hc, int wc, int blocks_x, int reg_vec) {
    __shared__ __attribute__((aligned(16))) float S[LH][LWV];
    __shared__ __attribute__((aligned(16))) float Hm[LH][TW];
    __shared__ AxisEntry XT[LWV], YT[LH];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int tx0 = (blockIdx.x % blocks_x) * TW;
    const int ty0 = (blockIdx.x / blocks_x) * TH;
    if (tid < LWV) XT[tid] = axis_entry(tx0 + tid - OFF, w, o, Tx, wc);
    else if (tid < LWV + LH) YT[tid - LWV] = axis_entry(ty0 + (tid - LWV) - HALO, h, o, Ty, hc);
    __syncthreads();
    const int xstep = w - o, ystep = h - o;

    if ((int)blockIdx.y >= C) {
        // regression plane: a bit copy from the owner tile, four adjacent cells of one row per thread
        const int rc = blockIdx.y - C, R = gridDim.y - C;
        const int r = tid / (TW / 4), c4 = (tid - r * (TW / 4)) * 4;
        const int y = ty0 + r, x = tx0 + c4;
        if (y >= hc || x >= wc) return;
        const AxisEntry ey = YT[r + HALO];
        float val[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const AxisEntry ex = XT[c4 + k + OFF];
            val[k] = 0.0f;
            if (ex.hi >= 0) {
                const int t = ey.own * Tx + ex.own;
                val[k] = reg[((int64_t)t * B + b) * r_sb + (int64_t)rc * r_sc + (int64_t)ey.own_l * w + ex.own_l];
            }
        }
        float* dst = out_reg + (((int64_t)b * R + rc) * hc + y) * wc + x;
        if (reg_vec) {
            *reinterpret_cast<float4*>(dst) = make_float4(val[0], val[1], val[2], val[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < wc) dst[k] = val[k];
        }
        return;
    }

    const int c = blockIdx.y;
    const float* base = hm + (int64_t)b * sb + (int64_t)c * sc;       // tile t's plane: base + t*B*sb
    const int64_t st = (int64_t)B * sb;
    // all loads of the thread are issued before the first use; contributions that do not exist read element 0 of tile 0's plane
    if (VEC) {
        constexpr int GR = LWV / 4, NG = LH * GR;                      // 18 groups per row, 360 per block
        constexpr int NLD = (NG + 255) / 256;
        float4 ld[NLD][4];
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * 256;
            const int r = min(i / GR, LH - 1), q = i - (i / GR) * GR;
            const AxisEntry ey = YT[r], ex = XT[4 * q];
            const bool ok = i < NG && ey.hi >= 0 && ex.hi >= 0;
            const bool ty2 = ok && ey.two, tx2 = ok && ex.two;
            const int64_t p_hh = ((int64_t)ey.hi * Tx + ex.hi) * st + (int64_t)ey.l * w + ex.l;
            const int64_t dy = (int64_t)Tx * st - (int64_t)ystep * w, dx = st - xstep;      // one tile down / left: same canvas cell
            ld[j][0] = *reinterpret_cast<const float4*>(base + (ty2 && tx2 ? p_hh - dy - dx : 0));
            ld[j][1] = *reinterpret_cast<const float4*>(base + (ty2 ? p_hh - dy : 0));
            ld[j][2] = *reinterpret_cast<const float4*>(base + (tx2 ? p_hh - dx : 0));
            ld[j][3] = *reinterpret_cast<const float4*>(base + (ok ? p_hh : 0));
        }
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * 256;
            const int r = min(i / GR, LH - 1), q = i - (i / GR) * GR;
            const AxisEntry ey = YT[r];
            const bool ok = ey.hi >= 0 && XT[4 * q].hi >= 0;
            float m[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const AxisEntry ex = XT[4 * q + k];
                const float v0 = k == 0 ? ld[j][0].x : k == 1 ? ld[j][0].y : k == 2 ? ld[j][0].z : ld[j][0].w;
                const float v1 = k == 0 ? ld[j][1].x : k == 1 ? ld[j][1].y : k == 2 ? ld[j][1].z : ld[j][1].w;
                const float v2 = k == 0 ? ld[j][2].x : k == 1 ? ld[j][2].y : k == 2 ? ld[j][2].z : ld[j][2].w;
                const float v3 = k == 0 ? ld[j][3].x : k == 1 ? ld[j][3].y : k == 2 ? ld[j][3].z : ld[j][3].w;
                float a = 0.0f;                                         // 0 + c is c: the sum starts at the first covering tile
                if (ey.two && ex.two) a = a + (ey.w_lo * ex.w_lo) * clamped_sigmoid(v0);
                if (ey.two)           a = a + (ey.w_lo * ex.w_hi) * clamped_sigmoid(v1);
                if (ex.two)           a = a + (ey.w_hi * ex.w_lo) * clamped_sigmoid(v2);
                a = a + (ey.w_hi * ex.w_hi) * clamped_sigmoid(v3);
                m[k] = ok ? a : -INFINITY;
            }
            if (i < NG) *reinterpret_cast<float4*>(&S[r][4 * q]) = make_float4(m[0], m[1], m[2], m[3]);
        }
    } else {
        constexpr int NC = LH * LWS;
        constexpr int NLD = (NC + 255) / 256;
        float ld[NLD][4];
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * 256;
            const int r = min(i / LWS, LH - 1), cc = i - (i / LWS) * LWS + OFF - HALO;
            const AxisEntry ey = YT[r], ex = XT[cc];
            const bool ok = i < NC && ey.hi >= 0 && ex.hi >= 0;
            const bool ty2 = ok && ey.two, tx2 = ok && ex.two;
            const int64_t p_hh = ((int64_t)ey.hi * Tx + ex.hi) * st + (int64_t)ey.l * w + ex.l;
            const int64_t dy = (int64_t)Tx * st - (int64_t)ystep * w, dx = st - xstep;
            ld[j][0] = base[ty2 && tx2 ? p_hh - dy - dx : 0];
            ld[j][1] = base[ty2 ? p_hh - dy : 0];
            ld[j][2] = base[tx2 ? p_hh - dx : 0];
            ld[j][3] = base[ok ? p_hh : 0];
        }
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * 256;
            const int r = min(i / LWS, LH - 1), cc = i - (i / LWS) * LWS + OFF - HALO;
            const AxisEntry ey = YT[r], ex = XT[cc];
            const bool ok = ey.hi >= 0 && ex.hi >= 0;
            float a = 0.0f;
            if (ey.two && ex.two) a = a + (ey.w_lo * ex.w_lo) * clamped_sigmoid(ld[j][0]);
            if (ey.two)           a = a + (ey.w_lo * ex.w_hi) * clamped_sigmoid(ld[j][1]);
            if (ex.two)           a = a + (ey.w_hi * ex.w_lo) * clamped_sigmoid(ld[j][2]);
            a = a + (ey.w_hi * ex.w_hi) * clamped_sigmoid(ld[j][3]);
            if (i < NC) S[r][cc] = ok ? a : -INFINITY;
        }
    }
    __syncthreads();
    nms5_tile_store(S, Hm, tid, ty0, tx0, hc, wc, out_hm + ((int64_t)b * C + c) * hc * wc, VEC);
}

// the geometry both entry points share: T tiles of n with overlap o along an axis
static int check_grid(const char* fn, int n_h, int n_w, int Ty, int Tx, int o) {
    SD_REQUIRE(Tx >= 1 && Tx <= 8 && Ty >= 1 && Ty <= 8, SD_ERR_INVALID, "%s: %d x %d tiles (1 .. 8 per axis are supported)", fn, Tx, Ty);
    SD_REQUIRE(o >= 0 && 2 * (int64_t)o <= (n_h < n_w ? n_h : n_w), SD_ERR_INVALID,
               "%s: overlap %d must satisfy 0 <= 2 * overlap <= min(%d, %d)", fn, o, n_h, n_w);
    return 0;
}

}  // namespace sd

using namespace sd;

extern "C" {

int sd_tile_views(const float* canvas, float* out, int B, int Hc, int Wc, int H, int W, int Ty, int Tx, int O, sd_stream_t stream) {
    const char* fn = "sd_tile_views";
    SD_REQUIRE(canvas != nullptr && out != nullptr, SD_ERR_INVALID, "%s: null pointer", fn);
    SD_REQUIRE(B > 0 && H > 0 && W > 0, SD_ERR_INVALID, "%s: bad tile shape (%d,3,%d,%d)", fn, B, H, W);
    if (int e = check_grid(fn, H, W, Ty, Tx, O)) return e;
    SD_REQUIRE((int64_t)Wc == (int64_t)Tx * W - (int64_t)(Tx - 1) * O && (int64_t)Hc == (int64_t)Ty * H - (int64_t)(Ty - 1) * O, SD_ERR_INVALID,
               "%s: canvas %d x %d is not %d x %d tiles of %d x %d with overlap %d (%lld x %lld)", fn, Wc, Hc, Tx, Ty, W, H, O,
               (long long)Tx * W - (long long)(Tx - 1) * O, (long long)Ty * H - (long long)(Ty - 1) * O);
    const bool vec = W % 4 == 0 && O % 4 == 0 && Wc % 4 == 0 && aligned16(canvas) && aligned16(out);
    const int64_t n = (int64_t)Ty * Tx * B * 3 * H * (vec ? W / 4 : W);
    const int64_t blocks = (n + 255) / 256;
    SD_REQUIRE(blocks < (1ll << 31), SD_ERR_INVALID, "%s: %lld blocks exceed the grid", fn, (long long)blocks);
    const dim3 grid((unsigned)blocks), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL((k_tile_views<true>), grid, block, 0, st, canvas, out, n, B, Hc, Wc, H, W, Tx, O);
    else     hipLaunchKernelGGL((k_tile_views<false>), grid, block, 0, st, canvas, out, n, B, Hc, Wc, H, W, Tx, O);
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_tile_merge_nms(const float* hm, int64_t sb, int64_t sc, int C, const float* reg, int64_t r_sb, int64_t r_sc, int R, float* out_hm,
                      float* out_reg, int B, int h, int w, int Ty, int Tx, int o, sd_stream_t stream) {
    const char* fn = "sd_tile_merge_nms";
    SD_REQUIRE(hm != nullptr && out_hm != nullptr, SD_ERR_INVALID, "%s: null pointer", fn);
    SD_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0, SD_ERR_INVALID, "%s: bad shape (%d,%d,%d,%d)", fn, B, C, h, w);
    SD_REQUIRE(R >= 0, SD_ERR_INVALID, "%s: R=%d regression channels", fn, R);
    SD_REQUIRE(R == 0 || (reg != nullptr && out_reg != nullptr), SD_ERR_INVALID, "%s: R=%d regression channels with a null pointer", fn, R);
    if (int e = check_grid(fn, h, w, Ty, Tx, o)) return e;
    const int64_t hc = (int64_t)Ty * h - (int64_t)(Ty - 1) * o, wc = (int64_t)Tx * w - (int64_t)(Tx - 1) * o;
    SD_REQUIRE(((int64_t)C + R) * hc * wc < (1ll << 31), SD_ERR_INVALID, "%s: (C+R)*hc*wc must be < 2^31", fn);
    SD_REQUIRE(sc >= (int64_t)h * w && sb >= (int64_t)h * w, SD_ERR_INVALID, "%s: bad strides sb=%lld sc=%lld", fn, (long long)sb,
               (long long)sc);
    SD_REQUIRE(R == 0 || (r_sc >= (int64_t)h * w && r_sb >= (int64_t)h * w), SD_ERR_INVALID, "%s: bad strides r_sb=%lld r_sc=%lld", fn,
               (long long)r_sb, (long long)r_sc);
    SD_REQUIRE(C + R <= 65535 && B <= 65535, SD_ERR_INVALID, "%s: B=%d, C+R=%d exceed the grid (65535)", fn, B, C + R);
    const int blocks_x = cdiv(wc, TW), blocks_y = cdiv(hc, TH);
    const bool vec = w % 4 == 0 && o % 4 == 0 && aligned16(hm) && aligned16(out_hm) && sb % 4 == 0 && sc % 4 == 0;
    const int reg_vec = R > 0 && wc % 4 == 0 && aligned16(out_reg);
    const dim3 grid(blocks_x * blocks_y, C + R, B), block(256);
    const hipStream_t st = (hipStream_t)stream;
    with_flag(vec, [&](auto vc) {
        hipLaunchKernelGGL((k_tile_merge_nms<decltype(vc)::value>), grid, block, 0, st, hm, sb, sc, C, reg, r_sb, r_sc, out_hm, out_reg, B, h, w,
                           Ty, Tx, o, (int)hc, (int)wc, blocks_x, reg_vec);
    });
    SD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
