// Cross-label anchor suppression for gfx950 (`--label_nms R`; no reference counterpart: the reference suppresses per heatmap channel only).
//   best(y,x) = max_c P[c,y,x], first(y,x) = the lowest c that attains it, win(y,x) = max of best over |dy|,|dx| <= R (cells outside the
//   map do not count), out[c,y,x] = (P[c,y,x] == win(y,x) && c == first(y,x)) ? P[c,y,x] : 0
// on the per-label suppressed probability maps P: what sd_nms5(apply_sigmoid = 1) or a merge kernel wrote.  Only max and == : the result is
// compared bit for bit with its definition.  (A second entry point that started from the head's logits and did the 5x5 NMS of every
// heatmap channel in the same launch was measured slower than sd_nms5 followed by this kernel and is not kept: DESIGN.md section 8.)
#include "sd_views.h"

namespace sd {

// ---------------------------------------------------------------------------------------------
// One 256-thread block per 64x16 tile of one image walks the M label channels (the tile of sd_nms5 and of the merge kernels).
//   per channel: the tile with a halo of R is staged in LDS (-inf outside the map), the loads of channel c + 1 are issued as soon as
//     channel c's values have left the registers; every thread keeps the running (Best, Arg) of its cells of the tile + R REGION in
//     registers, updated with a strict `>`: the lowest label wins.
//   after the loop: Best goes to LDS, the separable (2R+1)-max of it (row pass into Wm, column pass in registers) gives Win, and every
//     channel's tile is written as (Arg == c && Best == Win) ? Best : 0 -- four adjacent pixels of a row per thread, the input is never
//     read a second time.
// RM = the largest radius of the instantiation (2 or 8: the LDS arrays, the staging and the loop bounds are sized by it, the radius R <= RM
// itself is a run-time value and cells beyond it are neither loaded nor reduced); VEC = 16-byte loads and stores (w % 4 == 0, 16-byte aligned
// planes), else 4-byte.  All indices are relative to the RM-sized frame:
//   S[r][sc]       staged cell = region cell       y = ty0 - RM + r, x = tx0 - XO + sc        (XO = RM rounded up to 4)
//   region (r, q)  Best / Arg / Bm                 y = ty0 - RM + r, x = tx0 - RM + q         = S[r][q - RM + XO]
// ---------------------------------------------------------------------------------------------
template <int RM>
struct LabelTile {
    static constexpr int XO = (RM + 3) / 4 * 4;            // LDS column of map column tx0
    static constexpr int SW = TW + 2 * XO;                 // staged columns (VEC: all of them; scalar: XO - RM .. XO + TW + RM - 1)
    static constexpr int RRM = TH + 2 * RM, RCM = TW + 2 * RM;      // the region = the staged rows x the cells per row of the scalar variant
    static constexpr int NV = (RRM * (SW / 4) + 255) / 256;         // 16-byte groups a thread stages
    static constexpr int NS = (RRM * RCM + 255) / 256;              // 4-byte cells a thread stages = region cells a thread owns
    static constexpr int S_FLOATS = RRM * SW;                       // S; Bm (RRM x RCM) after the loop
};

template <int RM, bool VEC>
__global__ __launch_bounds__(256) void k_label_nms(const float* __restrict__ p, int64_t sb, int64_t sc, int M, int h, int w, int R, int tiles_x,
                                                   float* __restrict__ out) {
    using T = LabelTile<RM>;
    constexpr int XO = T::XO, SW = T::SW, RRM = T::RRM, RCM = T::RCM;
    __shared__ __attribute__((aligned(16))) float bufS[T::S_FLOATS];
    __shared__ __attribute__((aligned(16))) float Wm[RRM * TW];
    __shared__ int Am[TH][TW];
    const int tid = threadIdx.x;
    const int b = blockIdx.z;
    const int tx0 = (blockIdx.x % tiles_x) * TW;
    const int ty0 = (blockIdx.x / tiles_x) * TH;
    const float* img = p + (int64_t)b * sb;
    constexpr int NLD = VEC ? T::NV : T::NS;
    using LdT = std::conditional_t<VEC, float4, float>;
    LdT ld[NLD];

    // where item i of the staging lives: LDS offset, plane offset (0 for a cell that is not read), the predicates
    auto stage_cell = [&](int i, int& lds, int64_t& src, bool& in, bool& ok) {
        int r, scol;
        if (VEC) {
            constexpr int GR = SW / 4;
            r = i / GR;
            scol = 4 * (i - r * GR);
            in = i < RRM * GR;
        } else {
            r = i / RCM;
            scol = i - r * RCM + XO - RM;
            in = i < RRM * RCM;
        }
        const int y = ty0 - RM + r, x = tx0 - XO + scol;
        // inside the halo of this R (a 16-byte group: any of its four cells), and inside the map (a group lies entirely in or out)
        const bool need = y >= ty0 - R && y < ty0 + TH + R && x + (VEC ? 3 : 0) >= tx0 - R && x < tx0 + TW + R;
        ok = in && need && y >= 0 && y < h && x >= 0 && x < w;
        lds = r * SW + scol;
        src = ok ? (int64_t)y * w + x : 0;
    };
    auto load_channel = [&](int c) {
        const float* plane = img + (int64_t)c * sc;
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            int lds; int64_t src; bool in, ok;
            stage_cell(tid + j * 256, lds, src, in, ok);
            if constexpr (VEC) ld[j] = *reinterpret_cast<const float4*>(plane + src);
            else ld[j] = plane[src];
        }
    };

    // the region cells of the thread: cell j is (r, q) = ((tid + 256 j) / RCM, (tid + 256 j) % RCM); bit j of `act`: inside the R-region
    // and inside the map
    float Best[T::NS];
    int Arg[T::NS];
    unsigned act = 0;
#pragma unroll
    for (int j = 0; j < T::NS; ++j) {
        const int i = tid + j * 256;
        const int r = i / RCM, q = i - r * RCM;
        const int y = ty0 - RM + r, x = tx0 - RM + q;
        const bool a = i < RRM * RCM && r >= RM - R && r < RM + R + TH && q >= RM - R && q < RM + R + TW && y >= 0 && y < h && x >= 0 && x < w;
        act |= (a ? 1u : 0u) << j;
        Best[j] = -INFINITY;
        Arg[j] = 0;
    }

    load_channel(0);
    for (int c = 0; c < M; ++c) {
#pragma unroll
        for (int j = 0; j < NLD; ++j) {
            int lds; int64_t src; bool in, ok;
            stage_cell(tid + j * 256, lds, src, in, ok);
            if constexpr (VEC) {
                if (in) *reinterpret_cast<float4*>(&bufS[lds]) = ok ? ld[j] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            } else {
                if (in) bufS[lds] = ok ? ld[j] : -INFINITY;
            }
        }
        __syncthreads();
        if (c + 1 < M) load_channel(c + 1);                            // in flight while this channel is reduced
#pragma unroll
        for (int j = 0; j < T::NS; ++j) {
            if (act >> j & 1) {
                const int i = tid + j * 256;
                const int r = i / RCM, q = i - r * RCM;
                const float v = bufS[r * SW + q - RM + XO];
                if (v > Best[j]) {                                     // strict: a tie of labels stays with the lowest one
                    Best[j] = v;
                    Arg[j] = c;
                }
            }
        }
        __syncthreads();                                               // S is rewritten by the next channel (by Bm after the last)
    }

    // Bm = Best over the region (-inf outside the map and beyond R), the labels of the tile's own cells
    float* Bm = bufS;
#pragma unroll
    for (int j = 0; j < T::NS; ++j) {
        const int i = tid + j * 256;
        const int r = i / RCM, q = i - r * RCM;
        if (i < RRM * RCM) {
            Bm[i] = Best[j];
            if (r >= RM && r < RM + TH && q >= RM && q < RM + TW) Am[r - RM][q - RM] = Arg[j];
        }
    }
    __syncthreads();
    // row pass of the (2R+1)-max: Wm[r][cc] = max over map columns x-R .. x+R of tile column cc, on the region rows of this R
    for (int i = tid; i < RRM * TW; i += 256) {
        const int r = i / TW, cc = i - r * TW;
        if (r >= RM - R && r < RM + R + TH) {
            const float* s = &Bm[r * RCM + cc + RM];
            float m = s[0];
            for (int k = 1; k <= R; ++k) m = fmaxf(m, fmaxf(s[-k], s[k]));
            Wm[i] = m;
        }
    }
    __syncthreads();
    // column pass + output
    const int tr = tid / (TW / 4), c4 = (tid - tr * (TW / 4)) * 4;
    const int y = ty0 + tr, x = tx0 + c4;
    if (y >= h || x >= w) return;
    float best[4];
    int lab[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float* s = &Wm[(tr + RM) * TW + c4 + k];
        float m = s[0];
        for (int d = 1; d <= R; ++d) m = fmaxf(m, fmaxf(s[-d * TW], s[d * TW]));
        best[k] = Bm[(tr + RM) * RCM + c4 + k + RM];
        lab[k] = (best[k] == m) ? Am[tr][c4 + k] : -1;                 // -1: suppressed by a neighbour (a cell beyond the map's edge is not stored below)
    }
    float* dst = out + (int64_t)b * M * h * w + (int64_t)y * w + x;
    for (int c = 0; c < M; ++c, dst += (int64_t)h * w) {
        if (VEC) {
            *reinterpret_cast<float4*>(dst) = make_float4(lab[0] == c ? best[0] : 0.0f, lab[1] == c ? best[1] : 0.0f, lab[2] == c ? best[2] : 0.0f,
                                                          lab[3] == c ? best[3] : 0.0f);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (x + k < w) dst[k] = lab[k] == c ? best[k] : 0.0f;
        }
    }
}

constexpr int LABEL_NMS_MAX_R = 8, LABEL_NMS_MAX_M = 256;

}  // namespace sd

using namespace sd;

extern "C" {

int sd_label_nms(const float* p, int64_t sb, int64_t sc, float* out, int B, int M, int h, int w, int R, sd_stream_t stream) {
    const char* fn = "sd_label_nms";
    SD_REQUIRE(p != nullptr && out != nullptr, SD_ERR_INVALID, "%s: null pointer", fn);
    SD_REQUIRE(B > 0 && h > 0 && w > 0, SD_ERR_INVALID, "%s: bad shape (%d,%d,%d,%d)", fn, B, M, h, w);
    SD_REQUIRE(R >= 1 && R <= LABEL_NMS_MAX_R, SD_ERR_INVALID, "%s: R=%d (a radius of 1 .. %d cells is supported)", fn, R, LABEL_NMS_MAX_R);
    SD_REQUIRE(M >= 1 && M <= LABEL_NMS_MAX_M, SD_ERR_INVALID, "%s: M=%d labels (1 .. %d are supported)", fn, M, LABEL_NMS_MAX_M);
    SD_REQUIRE((int64_t)M * h * w < (1ll << 31), SD_ERR_INVALID, "%s: M*h*w must be < 2^31", fn);
    SD_REQUIRE(sc >= (int64_t)h * w && sb >= (int64_t)h * w, SD_ERR_INVALID, "%s: bad strides sb=%lld sc=%lld", fn, (long long)sb, (long long)sc);
    SD_REQUIRE(B <= 65535, SD_ERR_INVALID, "%s: B=%d exceeds the grid (65535)", fn, B);
    const int tiles_x = cdiv(w, TW), tiles_y = cdiv(h, TH);
    const bool vec = (w % 4 == 0) && aligned16(p) && aligned16(out) && sb % 4 == 0 && sc % 4 == 0;
    const dim3 grid(tiles_x * tiles_y, 1, B);
    const hipStream_t st = (hipStream_t)stream;
    with_flag(R <= 2, [&](auto small) {
        with_flag(vec, [&](auto vc) {
            constexpr int RM = decltype(small)::value ? 2 : LABEL_NMS_MAX_R;
            hipLaunchKernelGGL((k_label_nms<RM, decltype(vc)::value>), grid, dim3(256), 0, st, p, sb, sc, M, h, w, R, tiles_x, out);
        });
    });
    SD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
