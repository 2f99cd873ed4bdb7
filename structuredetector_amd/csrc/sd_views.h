// What the merge + NMS files share (sd_tta.hip: the flip views, sd_d4.hip: the transposed views, sd_tiles.hip: the tile stitch): the view
// table and its host check, the tile of the merge + NMS kernels, the staging of the mirrored views into that tile, its 5x5 NMS tail, the
// common argument checks of the merge entry points and the run-time -> template-constant dispatch of their launches.
#pragma once
#include <type_traits>

#include "sd_common.h"

namespace sd {

struct ViewFlips {
    unsigned char f[4];          // bit 0 = horizontal, bit 1 = vertical (the encoding of sd_preprocess_images' `flips`)
};

// One 256-thread block per 64x16 output tile of one merged map (the tile of sd_nms5), staged with its 2-pixel halo.
// LDS column of map column x: x - tx0 + OFF (OFF = 4) in the 16-byte and the 4-byte variants.
constexpr int TW = 64, TH = 16, HALO = 2, OFF = 4;
constexpr int LH = TH + 2 * HALO;        // 20 staged rows
constexpr int LWV = TW + 2 * OFF;        // 72 staged columns (VEC); the scalar variant fills columns OFF-HALO .. OFF+TW+HALO-1
constexpr int LWS = TW + 2 * HALO;       // 68 cells per row loaded by the scalar variant
constexpr int NLDV = (LH * (LWV / 4) + 255) / 256;      // 16-byte groups (18 per row, 360 per tile) a thread stages
constexpr int NLDS = (LH * LWS + 255) / 256;            // 4-byte cells (1360 per tile) a thread stages

__device__ __forceinline__ float4 reversed(const float4 v) { return make_float4(v.w, v.z, v.y, v.x); }

// ---------------------------------------------------------------------------------------------
// Staging of V mirrored views into the tile, in two steps so that a kernel can keep the loads in flight across other work: plain_load_*
// issues every load of the thread (cells outside the map read element 0), plain_sum_* gives s_0 + s_1 [+ s_2 + s_3] of one loaded
// item, s_v = clamped_sigmoid(view v's logit at the mirrored coordinate), summed in view order.  plain_cell_* places item i of the
// block: `in` = the item exists, `ok` = it exists and lies inside the map; S[r][c] is its LDS cell (the first of four for a group).
//   _vec: w % 4 == 0 and 16-byte aligned planes.  The staged span of a row is widened to the enclosing aligned groups [tx0-4, tx0+68);
//         a mirrored view reads the group w-4-x reversed, so its span is contiguous as well.  A group lies entirely inside or outside.
//   _scalar: one 4-byte load per staged cell, [tx0-2, tx0+66).
// ---------------------------------------------------------------------------------------------
struct TileCell {
    int r, c, y, x;
    bool in, ok;
};

__device__ __forceinline__ TileCell plain_cell_vec(int i, int ty0, int tx0, int h, int w) {
    constexpr int GR = LWV / 4;
    TileCell t;
    t.r = i / GR;
    t.c = 4 * (i - t.r * GR);
    t.y = ty0 + t.r - HALO;
    t.x = tx0 - OFF + t.c;
    t.in = i < LH * GR;
    t.ok = t.in && t.y >= 0 && t.y < h && t.x >= 0 && t.x < w;
    return t;
}

__device__ __forceinline__ TileCell plain_cell_scalar(int i, int ty0, int tx0, int h, int w) {
    TileCell t;
    t.r = i / LWS;
    t.c = i - t.r * LWS + OFF - HALO;
    t.y = ty0 + t.r - HALO;
    t.x = tx0 - OFF + t.c;
    t.in = i < LH * LWS;
    t.ok = t.in && t.y >= 0 && t.y < h && t.x >= 0 && t.x < w;
    return t;
}

template <int V>
__device__ __forceinline__ void plain_load_vec(float4 (&ld)[NLDV][V], const float* (&plane)[V], const ViewFlips& vf, int tid, int ty0, int tx0,
                                               int h, int w) {
#pragma unroll
    for (int j = 0; j < NLDV; ++j) {
        const TileCell t = plain_cell_vec(tid + j * 256, ty0, tx0, h, w);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int sy = (vf.f[v] & 2) ? h - 1 - t.y : t.y;
            const int sx = (vf.f[v] & 1) ? w - 4 - t.x : t.x;
            ld[j][v] = *reinterpret_cast<const float4*>(plane[v] + (t.ok ? (int64_t)sy * w + sx : 0));
        }
    }
}

template <int V>
__device__ __forceinline__ void plain_load_scalar(float (&ld)[NLDS][V], const float* (&plane)[V], const ViewFlips& vf, int tid, int ty0, int tx0,
                                                  int h, int w) {
#pragma unroll
    for (int j = 0; j < NLDS; ++j) {
        const TileCell t = plain_cell_scalar(tid + j * 256, ty0, tx0, h, w);
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int sy = (vf.f[v] & 2) ? h - 1 - t.y : t.y;
            const int sx = (vf.f[v] & 1) ? w - 1 - t.x : t.x;
            ld[j][v] = plane[v][t.ok ? (int64_t)sy * w + sx : 0];
        }
    }
}

template <int V>
__device__ __forceinline__ float4 plain_sum_vec(const float4 (&ld)[V], const ViewFlips& vf) {
    float4 m;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const float4 t = (vf.f[v] & 1) ? reversed(ld[v]) : ld[v];
        const float4 s = make_float4(clamped_sigmoid(t.x), clamped_sigmoid(t.y), clamped_sigmoid(t.z), clamped_sigmoid(t.w));
        if (v == 0) m = s;
        else { m.x = m.x + s.x; m.y = m.y + s.y; m.z = m.z + s.z; m.w = m.w + s.w; }
    }
    return m;
}

template <int V>
__device__ __forceinline__ float plain_sum_scalar(const float (&ld)[V]) {
    float m = clamped_sigmoid(ld[0]);
#pragma unroll
    for (int v = 1; v < V; ++v) m = m + clamped_sigmoid(ld[v]);
    return m;
}

// ---------------------------------------------------------------------------------------------
// The NMS tail of a staged tile S (-inf outside the map; the caller's barrier after staging comes first): the 5-max is separable, row
// pass into Hm, column pass in registers; out = (m == max5x5(m)) ? m : 0, four adjacent pixels of one row per thread, one 16-byte store
// (vec: w % 4 == 0 and a 16-byte aligned plane) or four 4-byte stores.  dst_plane: the (h, w) output plane of the block.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void nms5_tile_store(const float (&S)[LH][LWV], float (&Hm)[LH][TW], int tid, int ty0, int tx0, int h, int w,
                                                float* __restrict__ dst_plane, bool vec) {
    // row pass: Hm[r][cc] = max over map columns tx0+cc-2 .. tx0+cc+2
    for (int i = tid; i < LH * TW; i += 256) {
        const int r = i / TW, cc = i - r * TW;
        const float* s = &S[r][cc + OFF - HALO];
        Hm[r][cc] = fmaxf(fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3])), s[4]);
    }
    __syncthreads();
    // column pass + output
    const int r = tid / (TW / 4), c4 = (tid - r * (TW / 4)) * 4;
    const int y = ty0 + r, x = tx0 + c4;
    if (y >= h) return;
    float val[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float m = fmaxf(fmaxf(Hm[r][c4 + k], Hm[r + 1][c4 + k]), fmaxf(Hm[r + 2][c4 + k], Hm[r + 3][c4 + k]));
        const float mx = fmaxf(m, Hm[r + 4][c4 + k]);
        const float v = S[r + HALO][c4 + k + OFF];
        val[k] = (v == mx) ? v : 0.0f;
    }
    float* dst = dst_plane + (int64_t)y * w + x;
    if (vec) {
        if (x < w) *reinterpret_cast<float4*>(dst) = make_float4(val[0], val[1], val[2], val[3]);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (x + k < w) dst[k] = val[k];
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static inline int check_views(const char* fn, int V, const unsigned char* view_flips, ViewFlips* vf, bool single_view = false) {
    SD_REQUIRE(V == 2 || V == 4 || (single_view && V == 1), SD_ERR_INVALID, "%s: V=%d views (%s are supported)", fn, V,
               single_view ? "1, 2 or 4" : "2 or 4");
    SD_REQUIRE(view_flips != nullptr, SD_ERR_INVALID, "%s: null view_flips", fn);
    *vf = ViewFlips{{0, 0, 0, 0}};
    for (int v = 0; v < V; ++v) {
        SD_REQUIRE(view_flips[v] < 4, SD_ERR_INVALID, "%s: view_flips[%d]=%d (bit 0 = horizontal, bit 1 = vertical)", fn, v, (int)view_flips[v]);
        vf->f[v] = view_flips[v];
    }
    SD_REQUIRE(view_flips[0] == 0, SD_ERR_INVALID, "%s: view 0 must be the unflipped image (view_flips[0]=%d)", fn, (int)view_flips[0]);
    return 0;
}

// what the view-merge entry points check alike, in their order: the (B, C, h, w) map, the view table, the 32-bit plane offsets
static inline int check_merge_args(const char* fn, int B, int C, int h, int w, int V, const unsigned char* view_flips, ViewFlips* vf,
                                   bool single_view) {
    SD_REQUIRE(B > 0 && C > 0 && h > 0 && w > 0, SD_ERR_INVALID, "%s: bad shape (%d,%d,%d,%d)", fn, B, C, h, w);
    if (int e = check_views(fn, V, view_flips, vf, single_view)) return e;
    SD_REQUIRE((int64_t)C * h * w < (1ll << 31), SD_ERR_INVALID, "%s: C*h*w must be < 2^31", fn);
    return 0;
}

// f(std::integral_constant<int, V>) for the checked V (2 or 4; 1 as well where SINGLE), f(std::bool_constant<b>): the template
// constants of a launch from their run-time values
template <bool SINGLE, class F>
static inline void with_views(int V, F&& f) {
    if constexpr (SINGLE) {
        if (V == 1) return f(std::integral_constant<int, 1>{});
    }
    if (V == 2) f(std::integral_constant<int, 2>{});
    else        f(std::integral_constant<int, 4>{});
}

template <class F>
static inline void with_flag(bool b, F&& f) {
    if (b) f(std::true_type{});
    else   f(std::false_type{});
}

}  // namespace sd
