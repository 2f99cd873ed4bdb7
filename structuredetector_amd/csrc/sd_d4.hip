// Transposed views for gfx950: the other four symmetries of the rectangle grid beside the flips of sd_tta.hip.  sd_d4_views writes the
// mirrored batch AND the mirrored transposed batch of an input, sd_d4_merge_nms merges the head outputs of both into ONE suppressed
// probability map, sd_transpose_select transposes the selected images of a square training batch.  No reference counterpart.  The merged
// value decides which pixels survive the NMS and is compared bit for bit with sums of sd_clamped_sigmoid outputs: separately rounded
// multiplies and adds -- floating-point contraction is OFF in this file.
//
// Every transposed plane goes through an LDS tile, so that the global loads AND the global stores run along the fast axis.  The tile has
// an odd dword pitch: LDS banks are 4 bytes wide and a 32-lane half of a wave is served per cycle from 32 of them (ds_read_b32 /
// ds_write_b32), so a column walk at pitch p visits the banks p * i mod 32 -- all distinct for odd p, ONE bank for p = 64.
#pragma clang fp contract(off)
#include "sd_views.h"

namespace sd {

// ---------------------------------------------------------------------------------------------
// The 64 x 64 transpose tile.  T[r][c] holds source row r0 + r, column c0 + c.
//   4-byte accesses: cell i of 4096 is (i / 64, i % 64) -- a wave moves one 256-byte row span, and reads a column of T at pitch 65
//     (banks (r + c) mod 32: no conflict).
//   16-byte accesses (a row length that is a multiple of 4 and 16-byte aligned planes): group i of 1024 is four consecutive cells of a
//     row.  The four cells of a group go to / come from T one dword at a time (the odd pitch leaves no 16-byte alignment), at banks
//     (4 q + k + r) mod 32 for group q of row r: 16 groups of ONE row reach only 8 banks.  vec_cell therefore gives a 32-lane half
//     8 groups of 4 rows -- banks 4 q' + r' + const, all distinct -- and a wave 128-byte spans of 4 rows, twice.
// ---------------------------------------------------------------------------------------------
constexpr int TS = 64, TP = TS + 1;

__device__ __forceinline__ void vec_cell(int i, int* r, int* q) {
    *r = ((i >> 6) << 2) | ((i >> 3) & 3);
    *q = (i & 7) | (((i >> 5) & 1) << 3);
}

// ---------------------------------------------------------------------------------------------
// Views.  One block per 64 x 64 tile of one input plane: the tile is read ONCE (contiguous spans), every plain view is written from
// registers as k_tta_views writes it, and every transposed view from the LDS tile: view k of the transposed (W, H) plane has
//   out_t[k][fy(x)][fx(y)] = in[y][x],   fy(x) = W-1-x if bit 1 of view k else x,   fx(y) = H-1-y if bit 0 else y
// (the flip acts on the transposed image).  VEC: W % 4 == 0 and x / out 16-byte aligned; VECT: H % 4 == 0 and out_t 16-byte aligned.
// ---------------------------------------------------------------------------------------------
template <int V, bool VEC, bool VECT>
__global__ __launch_bounds__(256) void k_d4_views(const float* __restrict__ x, float* __restrict__ out, float* __restrict__ out_t,
                                                  int64_t planes, int H, int W, int tiles_x, int tiles, ViewFlips vf) {
    __shared__ float T[TS][TP];
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x / tiles;
    const int t = (int)(blockIdx.x - plane * tiles);
    const int ty0 = (t / tiles_x) * TS, tx0 = (t % tiles_x) * TS;
    const float* src = x + plane * H * W;
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int r, q;
            vec_cell(tid + j * 256, &r, &q);
            const int y = ty0 + r, xx = tx0 + 4 * q;
            if (y < H && xx < W) {                                        // W % 4 == 0: a group is inside or outside the row
                const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)y * W + xx);
                T[r][4 * q] = v.x; T[r][4 * q + 1] = v.y; T[r][4 * q + 2] = v.z; T[r][4 * q + 3] = v.w;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const bool hf = vf.f[k] & 1;
                    const int dy = (vf.f[k] & 2) ? H - 1 - y : y;
                    const int dx = hf ? W - 4 - xx : xx;
                    *reinterpret_cast<float4*>(out + (((int64_t)k * planes + plane) * H + dy) * W + dx) = hf ? reversed(v) : v;
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = tid + j * 256;
            const int r = i >> 6, c = i & 63;
            const int y = ty0 + r, xx = tx0 + c;
            if (y < H && xx < W) {
                const float v = src[(int64_t)y * W + xx];
                T[r][c] = v;
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int dy = (vf.f[k] & 2) ? H - 1 - y : y;
                    const int dx = (vf.f[k] & 1) ? W - 1 - xx : xx;
                    out[(((int64_t)k * planes + plane) * H + dy) * W + dx] = v;
                }
            }
        }
    }
    __syncthreads();
    // the transposed plane: row = source column, column = source row
    if (VECT) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c, q;
            vec_cell(tid + j * 256, &c, &q);
            const int xx = tx0 + c, y = ty0 + 4 * q;
            if (xx < W && y < H) {                                        // H % 4 == 0
                const float4 v = make_float4(T[4 * q][c], T[4 * q + 1][c], T[4 * q + 2][c], T[4 * q + 3][c]);
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const bool hf = vf.f[k] & 1;
                    const int dy = (vf.f[k] & 2) ? W - 1 - xx : xx;
                    const int dx = hf ? H - 4 - y : y;
                    *reinterpret_cast<float4*>(out_t + (((int64_t)k * planes + plane) * W + dy) * H + dx) = hf ? reversed(v) : v;
                }
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = tid + j * 256;
            const int c = i >> 6, r = i & 63;
            const int xx = tx0 + c, y = ty0 + r;
            if (xx < W && y < H) {
                const float v = T[r][c];
#pragma unroll
                for (int k = 0; k < V; ++k) {
                    const int dy = (vf.f[k] & 2) ? W - 1 - xx : xx;
                    const int dx = (vf.f[k] & 1) ? H - 1 - y : y;
                    out_t[(((int64_t)k * planes + plane) * W + dy) * H + dx] = v;
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Transpose the selected images of a (B, P, S, S) batch.  One block per 64 x 64 tile of one plane; the selection byte is read once
// per block (the branch is uniform): a copied tile leaves from registers, a transposed one through the LDS tile to the mirrored
// tile position.  VEC: S % 4 == 0 and both pointers 16-byte aligned.
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void k_transpose_select(const float* __restrict__ x, float* __restrict__ out, int P, int S, int tiles_x,
                                                          int tiles, const unsigned char* __restrict__ sel) {
    __shared__ float T[TS][TP];
    const int tid = threadIdx.x;
    const int64_t plane = blockIdx.x / tiles;
    const int t = (int)(blockIdx.x - plane * tiles);
    const int ty0 = (t / tiles_x) * TS, tx0 = (t % tiles_x) * TS;
    const bool tr = sel[plane / P] & 1;                                   // the other bits are not ours
    const float* src = x + plane * S * S;
    float* dst = out + plane * S * S;
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int r, q;
            vec_cell(tid + j * 256, &r, &q);
            const int y = ty0 + r, xx = tx0 + 4 * q;
            if (y < S && xx < S) {
                const float4 v = *reinterpret_cast<const float4*>(src + (int64_t)y * S + xx);
                if (tr) { T[r][4 * q] = v.x; T[r][4 * q + 1] = v.y; T[r][4 * q + 2] = v.z; T[r][4 * q + 3] = v.w; }
                else *reinterpret_cast<float4*>(dst + (int64_t)y * S + xx) = v;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = tid + j * 256;
            const int r = i >> 6, c = i & 63;
            const int y = ty0 + r, xx = tx0 + c;
            if (y < S && xx < S) {
                const float v = src[(int64_t)y * S + xx];
                if (tr) T[r][c] = v;
                else dst[(int64_t)y * S + xx] = v;
            }
        }
    }
    if (!tr) return;                                                      // uniform over the block
    __syncthreads();
    if (VEC) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int c, q;
            vec_cell(tid + j * 256, &c, &q);
            const int xx = tx0 + c, y = ty0 + 4 * q;
            if (xx < S && y < S)
                *reinterpret_cast<float4*>(dst + (int64_t)xx * S + y) = make_float4(T[4 * q][c], T[4 * q + 1][c], T[4 * q + 2][c], T[4 * q + 3][c]);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int i = tid + j * 256;
            const int c = i >> 6, r = i & 63;
            const int xx = tx0 + c, y = ty0 + r;
            if (xx < S && y < S) dst[(int64_t)xx * S + y] = T[r][c];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Merge + NMS over the plain and the transposed views.  Block, tile and halo are k_tta_merge_nms's (sd_views.h): the plain views are
// staged exactly as there, A = s_0 + s_1 [+ s_2 + s_3] in registers.  The transposed views fill the same tile from their (w, h) planes:
// merged cell (y, x) takes view v's logit at row fy_v(x), column fx_v(y) of its plane (fy_v(x) = w-1-x if bit 1 else x, fx_v(y) = h-1-y
// if bit 0 else y), so the tile's footprint is 68 (72) plane rows of 20 (24) contiguous cells.  They are loaded along the plane's
// fast axis, summed in view order in registers (Bt = t_0 + t_1 [+ t_2 + t_3], t_v = clamped_sigmoid) and written ONCE to the LDS
// array Tt[x][y] at the odd pitch 25; the plain pass reads Tt down its columns and stages m = (A + Bt) * (1 / (2 V)).  The 5-max and
// the output are those of k_tta_merge_nms.
//   VEC : w % 4 == 0, hm / out planes and strides 16-byte aligned -- plain views by 16-byte loads, [tx0-4, tx0+68), 16-byte stores.
//   VECT: h % 4 == 0, hm_t planes and strides 16-byte aligned -- transposed rows by 16-byte loads over [ty0-4, ty0+20); a mirrored row
//         reads the group h-4-y and swaps its components.  4-byte loads over [ty0-2, ty0+18) otherwise.
// Tt row of map column x: x - tx0 + OFF; Tt column of map row y: y - ty0 + OFF.
// ---------------------------------------------------------------------------------------------
constexpr int TYV = TH + 2 * OFF;        // 24 cells per transposed row loaded by the 16-byte variant
constexpr int TTP = TYV + 1;             // the odd pitch of Tt

template <int V, bool VEC, bool VECT>
__global__ __launch_bounds__(256) void k_d4_merge_nms(const float* __restrict__ hm, int64_t sb, int64_t sc, const float* __restrict__ hm_t,
                                                      int64_t sbt, int64_t sct, int B, int C, int h, int w, int tiles_x, ViewFlips vf,
                                                      float* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) float S[LH][LWV];
    __shared__ __attribute__((aligned(16))) float Hm[LH][TW];
    __shared__ float Tt[LWV][TTP];
    constexpr float inv = 0.5f / V;                                    // 0.5, 0.25, 0.125: exact
    constexpr int XN = VEC ? LWV : LWS;                                // map columns the plain pass stages, from tx0 - XO
    constexpr int XO = VEC ? OFF : HALO;
    const int tid = threadIdx.x;
    const int b = blockIdx.z, c = blockIdx.y;
    const int tx0 = (blockIdx.x % tiles_x) * TW;
    const int ty0 = (blockIdx.x / tiles_x) * TH;
    const float* plane[V];
    const float* plane_t[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
        plane[v] = hm + ((int64_t)v * B + b) * sb + (int64_t)c * sc;
        plane_t[v] = hm_t + ((int64_t)v * B + b) * sbt + (int64_t)c * sct;
    }

    // ---- transposed views -> Tt (cells outside the map read element 0 and are not written: the plain pass makes them -inf)
    if (VECT) {
        constexpr int GT = TYV / 4, NG = XN * GT;                      // 6 groups per plane row
        constexpr int NLD = (NG + 255) / 256;
        float4 ld[NLD][V];
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * 256;
            const int xr = i / GT, g = i - xr * GT;
            const int x = tx0 - XO + xr, y = ty0 - OFF + 4 * g;
            const bool ok = i < NG && x >= 0 && x < w && y >= 0 && y < h;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int sx = (vf.f[v] & 2) ? w - 1 - x : x;
                const int sy = (vf.f[v] & 1) ? h - 4 - y : y;
                ld[j][v] = *reinterpret_cast<const float4*>(plane_t[v] + (ok ? (int64_t)sx * h + sy : 0));
            }
        }
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * 256;
            const int xr = i / GT, g = i - xr * GT;
            const int x = tx0 - XO + xr, y = ty0 - OFF + 4 * g;
            const bool ok = i < NG && x >= 0 && x < w && y >= 0 && y < h;
            float4 m;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const float4 t = (vf.f[v] & 1) ? reversed(ld[j][v]) : ld[j][v];
                const float4 s = make_float4(clamped_sigmoid(t.x), clamped_sigmoid(t.y), clamped_sigmoid(t.z), clamped_sigmoid(t.w));
                if (v == 0) m = s;
                else { m.x = m.x + s.x; m.y = m.y + s.y; m.z = m.z + s.z; m.w = m.w + s.w; }
            }
            if (ok) {
                float* d = &Tt[xr + OFF - XO][4 * g];
                d[0] = m.x; d[1] = m.y; d[2] = m.z; d[3] = m.w;
            }
        }
    } else {
        constexpr int NC = XN * LH;
        constexpr int NLD = (NC + 255) / 256;
        float ld[NLD][V];
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * 256;
            const int xr = i / LH, yr = i - xr * LH;
            const int x = tx0 - XO + xr, y = ty0 - HALO + yr;
            const bool ok = i < NC && x >= 0 && x < w && y >= 0 && y < h;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int sx = (vf.f[v] & 2) ? w - 1 - x : x;
                const int sy = (vf.f[v] & 1) ? h - 1 - y : y;
                ld[j][v] = plane_t[v][ok ? (int64_t)sx * h + sy : 0];
            }
        }
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            const int i = tid + j * 256;
            const int xr = i / LH, yr = i - xr * LH;
            const int x = tx0 - XO + xr, y = ty0 - HALO + yr;
            const bool ok = i < NC && x >= 0 && x < w && y >= 0 && y < h;
            float m = clamped_sigmoid(ld[j][0]);
#pragma unroll
            for (int v = 1; v < V; ++v) m = m + clamped_sigmoid(ld[j][v]);
            if (ok) Tt[xr + OFF - XO][yr + OFF - HALO] = m;
        }
    }

    // ---- plain views (k_tta_merge_nms's staging, sd_views.h); their loads are in flight across the barrier
    if (VEC) {
        float4 ld[NLDV][V];
        plain_load_vec(ld, plane, vf, tid, ty0, tx0, h, w);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NLDV; ++j) {
            const TileCell t = plain_cell_vec(tid + j * 256, ty0, tx0, h, w);
            float4 m = plain_sum_vec(ld[j], vf);
            if (t.ok) {
                const int ry = t.r + OFF - HALO;
                m.x = (m.x + Tt[t.c][ry]) * inv; m.y = (m.y + Tt[t.c + 1][ry]) * inv;
                m.z = (m.z + Tt[t.c + 2][ry]) * inv; m.w = (m.w + Tt[t.c + 3][ry]) * inv;
            } else {
                m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            }
            if (t.in) *reinterpret_cast<float4*>(&S[t.r][t.c]) = m;
        }
    } else {
        float ld[NLDS][V];
        plain_load_scalar(ld, plane, vf, tid, ty0, tx0, h, w);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NLDS; ++j) {
            const TileCell t = plain_cell_scalar(tid + j * 256, ty0, tx0, h, w);
            const float m = plain_sum_scalar(ld[j]);
            if (t.in) S[t.r][t.c] = t.ok ? (m + Tt[t.c][t.r + OFF - HALO]) * inv : -INFINITY;
        }
    }
    __syncthreads();
    nms5_tile_store(S, Hm, tid, ty0, tx0, h, w, out + ((int64_t)b * C + c) * h * w, VEC);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static bool ranges_overlap(const float* a, const float* b, int64_t n) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b), bytes = (uintptr_t)n * sizeof(float);
    return pa < pb + bytes && pb < pa + bytes;
}

}  // namespace sd

using namespace sd;

extern "C" {

int sd_d4_views(const float* x, float* out, float* out_t, int B, int H, int W, int Vf, const unsigned char* view_flips_host,
                sd_stream_t stream) {
    const char* fn = "sd_d4_views";
    SD_REQUIRE(x != nullptr && out != nullptr && out_t != nullptr, SD_ERR_INVALID, "%s: null pointer", fn);
    SD_REQUIRE(B > 0 && H > 0 && W > 0, SD_ERR_INVALID, "%s: bad shape (%d,3,%d,%d)", fn, B, H, W);
    ViewFlips vf;
    if (int e = check_views(fn, Vf, view_flips_host, &vf, true)) return e;
    SD_REQUIRE((int64_t)3 * H * W < (1ll << 31), SD_ERR_INVALID, "%s: 3*H*W must be < 2^31", fn);
    const int64_t planes = (int64_t)B * 3;
    const int tiles_x = cdiv(W, TS), tiles = tiles_x * cdiv(H, TS);
    const int64_t blocks = planes * tiles;
    SD_REQUIRE(blocks < (1ll << 31), SD_ERR_INVALID, "%s: %lld blocks exceed the grid", fn, (long long)blocks);
    const bool vec = (W % 4 == 0) && aligned16(x) && aligned16(out);
    const bool vect = (H % 4 == 0) && aligned16(out_t);
    const dim3 grid((unsigned)blocks), block(256);
    const hipStream_t st = (hipStream_t)stream;
    with_views<true>(Vf, [&](auto v) {
        with_flag(vec, [&](auto vc) {
            with_flag(vect, [&](auto vt) {
                hipLaunchKernelGGL((k_d4_views<decltype(v)::value, decltype(vc)::value, decltype(vt)::value>), grid, block, 0, st, x, out, out_t,
                                   planes, H, W, tiles_x, tiles, vf);
            });
        });
    });
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_d4_merge_nms(const float* hm, int64_t sb, int64_t sc, const float* hm_t, int64_t sb_t, int64_t sc_t, float* out, int B, int C, int h,
                    int w, int Vf, const unsigned char* view_flips_host, sd_stream_t stream) {
    const char* fn = "sd_d4_merge_nms";
    SD_REQUIRE(hm != nullptr && hm_t != nullptr && out != nullptr, SD_ERR_INVALID, "%s: null pointer", fn);
    ViewFlips vf;
    if (int e = check_merge_args(fn, B, C, h, w, Vf, view_flips_host, &vf, true)) return e;
    SD_REQUIRE(sc >= (int64_t)h * w && sb >= (int64_t)h * w, SD_ERR_INVALID, "%s: bad strides sb=%lld sc=%lld", fn, (long long)sb, (long long)sc);
    SD_REQUIRE(sc_t >= (int64_t)h * w && sb_t >= (int64_t)h * w, SD_ERR_INVALID, "%s: bad strides sb_t=%lld sc_t=%lld", fn, (long long)sb_t,
               (long long)sc_t);
    SD_REQUIRE(C <= 65535 && B <= 65535, SD_ERR_INVALID, "%s: B=%d, C=%d exceed the grid (65535)", fn, B, C);
    const int tiles_x = cdiv(w, TW), tiles_y = cdiv(h, TH);
    const bool vec = (w % 4 == 0) && aligned16(hm) && aligned16(out) && sb % 4 == 0 && sc % 4 == 0;
    const bool vect = (h % 4 == 0) && aligned16(hm_t) && sb_t % 4 == 0 && sc_t % 4 == 0;
    const dim3 grid(tiles_x * tiles_y, C, B), block(256);
    const hipStream_t st = (hipStream_t)stream;
    with_views<true>(Vf, [&](auto v) {
        with_flag(vec, [&](auto vc) {
            with_flag(vect, [&](auto vt) {
                hipLaunchKernelGGL((k_d4_merge_nms<decltype(v)::value, decltype(vc)::value, decltype(vt)::value>), grid, block, 0, st, hm, sb, sc,
                                   hm_t, sb_t, sc_t, B, C, h, w, tiles_x, vf, out);
            });
        });
    });
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_transpose_select(const float* x, float* out, int B, int P, int S, const unsigned char* sel_dev, sd_stream_t stream) {
    const char* fn = "sd_transpose_select";
    SD_REQUIRE(x != nullptr && out != nullptr && sel_dev != nullptr, SD_ERR_INVALID, "%s: null pointer", fn);
    SD_REQUIRE(B > 0 && P > 0 && S > 0, SD_ERR_INVALID, "%s: bad shape (%d,%d,%d,%d)", fn, B, P, S, S);
    SD_REQUIRE((int64_t)P * S * S < (1ll << 31), SD_ERR_INVALID, "%s: P*S*S must be < 2^31", fn);
    const int64_t planes = (int64_t)B * P;
    SD_REQUIRE(!ranges_overlap(x, out, planes * S * S), SD_ERR_INVALID, "%s: x and out overlap (the transpose is not in place)", fn);
    const int tiles_x = cdiv(S, TS), tiles = tiles_x * tiles_x;
    const int64_t blocks = planes * tiles;
    SD_REQUIRE(blocks < (1ll << 31), SD_ERR_INVALID, "%s: %lld blocks exceed the grid", fn, (long long)blocks);
    const dim3 grid((unsigned)blocks), block(256);
    const hipStream_t st = (hipStream_t)stream;
    if ((S % 4 == 0) && aligned16(x) && aligned16(out)) hipLaunchKernelGGL((k_transpose_select<true>), grid, block, 0, st, x, out, P, S, tiles_x, tiles, sel_dev);
    else                                                hipLaunchKernelGGL((k_transpose_select<false>), grid, block, 0, st, x, out, P, S, tiles_x, tiles, sel_dev);
    SD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
