// Evaluation matching for gfx950: sd_eval_match labels EVERY top-k slot of a decoded batch a hit or a miss against the ground truth,
// the way Evaluator._accumulate_fast does for the anchor and the raw-part lists (greedy by descending score, a prediction only ever
// tries its NEAREST ground truth of its class).  Whether slot i is a hit depends only on the slots ranked above it, so one pass serves
// every confidence threshold: the host bins the slots by score and the counters at threshold t are prefix counts (model/pr_curve.py).
// No reference counterpart.  Coordinates and distances are fp64 with every multiply rounded separately, as the host computes them
// (`kp.x * sx` in Decoder._assemble, `* fx` in the Evaluator, np.hypot): floating-point contraction is OFF in this file.
//
// One 256-thread block per (image, list); a thread owns slots tid, tid + 256, ... (at most EVAL_SLOTS of them: K, P <= SD_MAX_TOPK).
// The segment's ground truths pass through LDS in chunks of EVAL_CHUNK; every thread walks a chunk front to back (all lanes read one
// LDS address: a broadcast) and keeps a running first minimum per slot.  The claim -- the LOWEST slot index among those nearest to one
// ground truth within the radius wins -- is an integer atomicMin on one LDS word per ground truth, a chunk of ground truths at a time:
// order-independent, so the result is deterministic.  Plain vector stores; no global atomics, no workspace.
#pragma clang fp contract(off)
#include "sd_common.h"

namespace sd {

constexpr int EVAL_THREADS = 256;
constexpr int EVAL_SLOTS = SD_MAX_TOPK / EVAL_THREADS;      // 4
constexpr int EVAL_CHUNK = SD_EVAL_GT_CHUNK;                // ground truths staged at once: 1024 x (8 + 8 + 4 + 4) bytes = 24 KB of LDS

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_match(const float* __restrict__ a_list, const float* __restrict__ p_list, int B, int K,
                                                             int P, const double* __restrict__ gt_xy, const int* __restrict__ gt_cls,
                                                             const int* __restrict__ gt_off, int G, const double* __restrict__ img,
                                                             double sx, double sy, int* __restrict__ match, double* __restrict__ dist) {
    __shared__ double gx[EVAL_CHUNK], gy[EVAL_CHUNK];
    __shared__ int gc[EVAL_CHUNK], win[EVAL_CHUNK];
    const int tid = threadIdx.x;
    const int b = blockIdx.x >> 1, part = blockIdx.x & 1;
    const int L = part ? P : K;
    const int seg = part ? B + b : b;
    // the offsets are device data the host cannot check without a wait: clamped into [0, G], so any table is memory-safe
    const int lo = min(max(gt_off[seg], 0), G);
    const int hi = min(max(gt_off[seg + 1], lo), G);
    const double fx = img[b * 3], fy = img[b * 3 + 1], thr = img[b * 3 + 2];

    double X[EVAL_SLOTS], Y[EVAL_SLOTS], best[EVAL_SLOTS];
    int cls[EVAL_SLOTS], bj[EVAL_SLOTS];
#pragma unroll
    for (int s = 0; s < EVAL_SLOTS; ++s) {
        const int i = tid + s * EVAL_THREADS;
        float x = 0.0f, y = 0.0f, c = -1.0f;
        if (i < L) {
            if (part) {
                const float* src = p_list + ((int64_t)b * P + i) * 6;            // 24-byte records: 8-byte aligned
                const float2 xy = *reinterpret_cast<const float2*>(src);
                const float2 sc = *reinterpret_cast<const float2*>(src + 2);
                x = xy.x; y = xy.y; c = sc.y;
            } else {
                const float4 v = *reinterpret_cast<const float4*>(a_list + ((int64_t)b * K + i) * 4);
                x = v.x; y = v.y; c = v.w;
            }
        }
        X[s] = ((double)x * sx) * fx;
        Y[s] = ((double)y * sy) * fy;
        cls[s] = i < L ? (int)c : -1;                                            // ground-truth classes are >= 0 where they count
        best[s] = INFINITY;
        bj[s] = -1;
    }

    // ---- nearest ground truth of the slot's class: first minimum over j ascending
    for (int c0 = lo; c0 < hi; c0 += EVAL_CHUNK) {
        const int n = min(EVAL_CHUNK, hi - c0);
        __syncthreads();                                                         // the previous chunk has been read
        for (int j = tid; j < n; j += EVAL_THREADS) {
            const double2 g = *reinterpret_cast<const double2*>(gt_xy + (int64_t)(c0 + j) * 2);
            gx[j] = g.x; gy[j] = g.y; gc[j] = gt_cls[c0 + j];
        }
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const double px = gx[j], py = gy[j];
            const int pc = gc[j];
#pragma unroll
            for (int s = 0; s < EVAL_SLOTS; ++s) {
                if (pc == cls[s] && pc >= 0) {
                    const double d = hypot(X[s] - px, Y[s] - py);
                    if (bj[s] < 0 || d < best[s]) { best[s] = d; bj[s] = c0 + j - lo; }
                }
            }
        }
    }

    // ---- claims: per ground truth the lowest slot index among those it is nearest to within the radius
    bool hit[EVAL_SLOTS];
#pragma unroll
    for (int s = 0; s < EVAL_SLOTS; ++s) hit[s] = false;
    for (int c0 = 0; c0 < hi - lo; c0 += EVAL_CHUNK) {
        __syncthreads();                                                         // gc / win of the pass before are no longer read
        for (int j = tid; j < EVAL_CHUNK; j += EVAL_THREADS) win[j] = 0x7fffffff;
        __syncthreads();
#pragma unroll
        for (int s = 0; s < EVAL_SLOTS; ++s) {
            const int r = bj[s] - c0;
            if (bj[s] >= 0 && r >= 0 && r < EVAL_CHUNK && best[s] < thr) atomicMin(&win[r], tid + s * EVAL_THREADS);
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < EVAL_SLOTS; ++s) {
            const int r = bj[s] - c0;
            if (bj[s] >= 0 && r >= 0 && r < EVAL_CHUNK && best[s] < thr && win[r] == tid + s * EVAL_THREADS) hit[s] = true;
        }
    }

    const int64_t row = (int64_t)b * (K + P) + (part ? K : 0);
#pragma unroll
    for (int s = 0; s < EVAL_SLOTS; ++s) {
        const int i = tid + s * EVAL_THREADS;
        if (i < L) {
            match[row + i] = hit[s] ? bj[s] : -1;
            dist[row + i] = bj[s] >= 0 ? best[s] : (double)INFINITY;
        }
    }
}

}  // namespace sd

using namespace sd;

extern "C" {

int sd_eval_match(const float* a_list, const float* p_list, int B, int K, int P, const double* gt_xy, const int* gt_cls, const int* gt_off,
                  int G, const double* img, double sx, double sy, int* match, double* dist, sd_stream_t stream) {
    const char* fn = "sd_eval_match";
    SD_REQUIRE(a_list != nullptr && p_list != nullptr && gt_xy != nullptr && gt_cls != nullptr && gt_off != nullptr && img != nullptr &&
               match != nullptr && dist != nullptr, SD_ERR_INVALID, "%s: null pointer", fn);
    SD_REQUIRE(B > 0 && K > 0 && P > 0, SD_ERR_INVALID, "%s: bad sizes B=%d K=%d P=%d", fn, B, K, P);
    SD_REQUIRE(K <= SD_MAX_TOPK && P <= SD_MAX_TOPK, SD_ERR_INVALID, "%s: K=%d, P=%d out of range (max %d)", fn, K, P, SD_MAX_TOPK);
    SD_REQUIRE(G >= 0, SD_ERR_INVALID, "%s: G=%d is negative", fn, G);
    SD_REQUIRE(B <= (1 << 29), SD_ERR_INVALID, "%s: B=%d exceeds the grid", fn, B);
    SD_REQUIRE(sx == sx && sy == sy, SD_ERR_INVALID, "%s: sx / sy is not a number", fn);
    const auto misaligned = [](const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; };
    SD_REQUIRE(!misaligned(a_list, 16) && !misaligned(p_list, 8) && !misaligned(gt_xy, 16) && !misaligned(gt_cls, 4) && !misaligned(gt_off, 4) &&
               !misaligned(img, 8) && !misaligned(match, 4) && !misaligned(dist, 8), SD_ERR_ALIGN,
               "%s: misaligned pointer (a_list, gt_xy: 16 bytes; p_list, img, dist: 8; gt_cls, gt_off, match: 4)", fn);
    hipLaunchKernelGGL(k_eval_match, dim3(2u * (unsigned)B), dim3(EVAL_THREADS), 0, (hipStream_t)stream, a_list, p_list, B, K, P, gt_xy, gt_cls,
                       gt_off, G, img, sx, sy, match, dist);
    SD_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
