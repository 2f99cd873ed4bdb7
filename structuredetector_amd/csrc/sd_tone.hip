// Histogram tone curves of 8-bit RGB images (`train --aug_equalize / --aug_autocontrast`; not in the reference): byte for byte Pillow's
// ImageOps.equalize(img) and ImageOps.autocontrast(img, cutoff).  Both are a 256-entry look-up table per image and channel, made from that
// channel's histogram h[0..255] of the n = H W pixels (tests/tone_ref.py restates both and is pinned against Pillow):
//     equalize:     fewer than two non-empty bins, or step = (n - h[highest non-empty bin]) / 255 == 0: the identity; else
//                   lut[i] = min(255, (step / 2 + h[0] + .. + h[i - 1]) / step), 32-bit unsigned integers;
//     autocontrast: lo = the value of the (cut_lo + 1)-th darkest pixel, hi = that of the (cut_hi + 1)-th brightest; cut_lo + cut_hi >= n
//                   or hi <= lo: the identity; else in IEEE double scale = 255.0 / (hi - lo), offset = -lo * scale and
//                   lut[i] = clamp(trunc(i * scale + offset), 0, 255), the product and the sum rounded one after the other (no FMA).
// table (B, 4) int32 on the device: [mode, cut_lo, cut_hi, 0]; mode 1 = autocontrast, 2 = equalize, anything else copies the image.  The
// table cannot be checked without a sync: the cuts are clamped to [0, n] and nothing in a row decides an address, so any table is safe.
//
// One memset of the histograms and two launches.  An image is a string of 3 n bytes whose byte o belongs to channel o mod 3; the kernels
// cut it into the bytes in front of the first 16-byte boundary (< 16), whole 16-byte chunks, and a tail (< 16).  Block x of an image owns
// TONE_CHUNKS chunks = SD_TONE_STRIP_PIXELS pixels; block 0 also takes the head and the tail, byte by byte.
// k_tone_hist (512 threads) counts into TONE_SUB sub-histograms of 3 x 256 bins in LDS, chosen by lane mod TONE_SUB and TONE_SUB_PITCH = 769
// words apart, so that the lanes of a wave that meet the same value -- flat content: letterbox bars, the warp's fill, sky -- still spread
// over TONE_SUB banks; and a lane first folds equal successive values of a channel within its chunk into one add of their count, which
// turns the 16 LDS atomics of a chunk into 3 on a flat frame.  The block then adds its non-zero bins to the image's (3, 256) uint32
// histogram in the workspace: integer sums, so the result does not depend on the order of arrival.
// k_tone_apply: three waves of every block scan the image's 3 x 256 counts (4 bins a lane, then a shuffle scan), evaluate the closed forms
// and leave the 768 table bytes in LDS (measured 3.5 us a call faster than a launch of its own that writes the tables to memory); the block
// then maps its strip chunk by chunk.  Every byte is read and written by the same thread, so out may be in.  When in and out differ in
// their offset from a 16-byte boundary the image is mapped byte by byte.
#include "sd_common.h"

namespace sd {

constexpr int TONE_CHUNKS = SD_TONE_STRIP_PIXELS * 3 / 16;               // 16-byte chunks of a block
constexpr int TONE_STRIP_BYTES = TONE_CHUNKS * 16;
constexpr int TONE_HT = 512, TONE_HU = 3;                                // k_tone_hist: threads of a block, chunks a thread has in flight
constexpr int TONE_SUB = 8, TONE_SUB_PITCH = 3 * 256 + 1;                // sub-histograms of a block and their distance in words
constexpr int TONE_UNROLL = 4;                                           // k_tone_apply: chunks a thread has in flight
constexpr size_t TONE_HIST_BYTES = 3 * 256 * sizeof(uint32_t);          // per image

__device__ __forceinline__ bool tone_on(int mode) { return mode == 1 || mode == 2; }

// the image's bytes as head | chunks x 16 | tail, by the address of its first byte
struct ToneSpan {
    int64_t head, chunks, tail_at;
    int tail;
};

__device__ __forceinline__ ToneSpan tone_span(const uint8_t* img, int64_t nb) {
    ToneSpan s;
    s.head = min((int64_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(img) & 15u)) & 15u), nb);
    s.chunks = (nb - s.head) >> 4;
    s.tail_at = s.head + 16 * s.chunks;
    s.tail = (int)(nb - s.tail_at);
    return s;
}

__device__ __forceinline__ uint32_t chunk_byte(const uint4& v, int k) {
    const uint32_t w = (k >> 2) == 0 ? v.x : (k >> 2) == 1 ? v.y : (k >> 2) == 2 ? v.z : v.w;
    return (w >> (8 * (k & 3))) & 255u;
}

// the bytes J, J + 3, .. of a chunk belong to one channel with the bins h: equal successive values are counted by one add
template <int J>
__device__ __forceinline__ void count_channel(uint32_t* h, const uint4& v) {
    uint32_t val = chunk_byte(v, J), cnt = 1;
#pragma unroll
    for (int k = J + 3; k < 16; k += 3) {
        const uint32_t x = chunk_byte(v, k);
        if (x == val) {
            ++cnt;
        } else {
            atomicAdd(&h[val], cnt);
            val = x;
            cnt = 1;
        }
    }
    atomicAdd(&h[val], cnt);
}

__global__ __launch_bounds__(TONE_HT) void k_tone_hist(const uint8_t* __restrict__ in, uint32_t* __restrict__ hist, int64_t nb,
                                                   const int* __restrict__ table) {
    const int b = blockIdx.y;
    if (!tone_on(table[4 * b])) return;                                  // uniform per block
    __shared__ uint32_t sh[TONE_SUB * TONE_SUB_PITCH];
    const int tid = threadIdx.x;
    for (int i = tid; i < TONE_SUB * TONE_SUB_PITCH; i += TONE_HT) sh[i] = 0;
    __syncthreads();
    const uint8_t* img = in + b * nb;
    const ToneSpan s = tone_span(img, nb);
    uint32_t* mine = sh + (tid & (TONE_SUB - 1)) * TONE_SUB_PITCH;
    const int64_t c0 = (int64_t)blockIdx.x * TONE_CHUNKS;                // a multiple of 3
    const int mine_chunks = (int)max((int64_t)0, min((int64_t)TONE_CHUNKS, s.chunks - c0));
    const uint4* src = reinterpret_cast<const uint4*>(img + s.head) + c0;
    for (int base = tid; base < mine_chunks; base += TONE_HT * TONE_HU) {
        uint4 v[TONE_HU];
#pragma unroll
        for (int u = 0; u < TONE_HU; ++u)
            if (base + TONE_HT * u < mine_chunks) v[u] = src[base + TONE_HT * u];
#pragma unroll
        for (int u = 0; u < TONE_HU; ++u)
            if (base + TONE_HT * u < mine_chunks) {
                const int p = ((int)s.head + base + TONE_HT * u) % 3;        // the channel of the chunk's byte 0: 16 c = c (mod 3)
                count_channel<0>(mine + 256 * p, v[u]);
                count_channel<1>(mine + 256 * (p == 2 ? 0 : p + 1), v[u]);
                count_channel<2>(mine + 256 * (p == 0 ? 2 : p - 1), v[u]);
            }
    }
    if (blockIdx.x == 0) {                                               // head and tail, a byte a thread
        if (tid < s.head) atomicAdd(&mine[256 * (tid % 3) + img[tid]], 1u);
        if (tid >= 16 && tid - 16 < s.tail) {
            const int64_t o = s.tail_at + (tid - 16);
            atomicAdd(&mine[256 * (int)(o % 3) + img[o]], 1u);
        }
    }
    __syncthreads();
    uint32_t* dst = hist + (size_t)b * 768;
    for (int i = tid; i < 768; i += TONE_HT) {
        uint32_t sum = 0;
#pragma unroll
        for (int k = 0; k < TONE_SUB; ++k) sum += sh[k * TONE_SUB_PITCH + i];
        if (sum) atomicAdd(&dst[i], sum);
    }
}

__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave: the table of one channel (its 256 counts hc) of image b, four entries a lane -- lane l holds the bins 4 l .. 4 l + 3
__device__ __forceinline__ uint32_t tone_lut_wave(const uint32_t* __restrict__ hc, uint32_t n, int mode, const int* __restrict__ table, int b,
                                                  int lane) {
    const uint4 hv = reinterpret_cast<const uint4*>(hc)[lane];
    const uint32_t h[4] = {hv.x, hv.y, hv.z, hv.w};
    uint32_t incl = h[0] + h[1] + h[2] + h[3];                           // inclusive scan of the lanes' sums
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    uint32_t below[4];                                                   // h[0] + .. + h[i - 1] of the lane's four bins
    below[0] = incl - (h[0] + h[1] + h[2] + h[3]);
    below[1] = below[0] + h[0];
    below[2] = below[1] + h[1];
    below[3] = below[2] + h[2];
    uint32_t r[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = 4 * lane + k;                     // the identity
    if (mode == 2) {
        int filled = 0, top = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (h[k]) {
                ++filled;
                top = 4 * lane + k;
            }
        filled = wave_sum_i(filled);
        top = wave_max_i(top);
        if (filled >= 2) {
            const uint32_t step = (n - hc[top]) / 255u;
            if (step)
#pragma unroll
                for (int k = 0; k < 4; ++k) r[k] = min(255u, (step / 2 + below[k]) / step);
        }
    } else {
        const uint32_t cut_lo = (uint32_t)min(max(table[4 * b + 1], 0), (int)n);   // n < 2^31
        const uint32_t cut_hi = (uint32_t)min(max(table[4 * b + 2], 0), (int)n);
        if (cut_lo + cut_hi < n) {
            int lo = 256, hi = -1;
#pragma unroll
            for (int k = 3; k >= 0; --k)
                if (below[k] + h[k] > cut_lo) lo = 4 * lane + k;         // h[0] + .. + h[i] > cut_lo: the smallest such i
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (n - below[k] > cut_hi) hi = 4 * lane + k;            // h[i] + .. + h[255] > cut_hi: the largest such i
            lo = wave_min_i(lo);
            hi = wave_max_i(hi);
            if (hi > lo) {
                const double scale = 255.0 / (double)(hi - lo);
                const double offset = __dmul_rn(-(double)lo, scale);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const double t = __dadd_rn(__dmul_rn((double)(4 * lane + k), scale), offset);
                    r[k] = (uint32_t)min(max((int)t, 0), 255);           // |t| <= 255 * 255: the conversion truncates towards zero
                }
            }
        }
    }
    return r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
}

// the waves 0 .. 2 of every block first make the image's three tables from its histogram, straight into LDS
__global__ __launch_bounds__(256) void k_tone_apply(const uint8_t* in, uint8_t* out, const uint32_t* __restrict__ hist, int64_t nb,
                                                    const int* __restrict__ table, int vec) {
    const int b = blockIdx.y;
    const int mode = table[4 * b];
    const bool on = tone_on(mode);
    if (!on && in == out) return;                                        // uniform per block
    __shared__ uint32_t sl[192];
    const int tid = threadIdx.x;
    if (on && tid < 192) sl[tid] = tone_lut_wave(hist + ((size_t)b * 3 + (tid >> 6)) * 256, (uint32_t)(nb / 3), mode, table, b, tid & 63);
    __syncthreads();
    const uint8_t* s8 = reinterpret_cast<const uint8_t*>(sl);
    const uint8_t* img = in + b * nb;
    uint8_t* dst = out + b * nb;
    if (!vec) {
        const int64_t o0 = (int64_t)blockIdx.x * TONE_STRIP_BYTES, o1 = min(o0 + TONE_STRIP_BYTES, nb);
        for (int64_t o = o0 + tid; o < o1; o += 256) dst[o] = on ? s8[256 * (int)(o % 3) + img[o]] : img[o];
        return;
    }
    const ToneSpan s = tone_span(img, nb);                               // dst has the same offset from a 16-byte boundary
    const int64_t c0 = (int64_t)blockIdx.x * TONE_CHUNKS;                // a multiple of 3
    const int mine_chunks = (int)max((int64_t)0, min((int64_t)TONE_CHUNKS, s.chunks - c0));
    const uint4* src = reinterpret_cast<const uint4*>(img + s.head) + c0;
    uint4* to = reinterpret_cast<uint4*>(dst + s.head) + c0;
    for (int base = tid; base < mine_chunks; base += 256 * TONE_UNROLL) {
        uint4 v[TONE_UNROLL];
#pragma unroll
        for (int u = 0; u < TONE_UNROLL; ++u)
            if (base + 256 * u < mine_chunks) v[u] = src[base + 256 * u];
#pragma unroll
        for (int u = 0; u < TONE_UNROLL; ++u)
            if (base + 256 * u < mine_chunks) {
                if (on) {
                    const int p = ((int)s.head + base + 256 * u) % 3;
                    const uint8_t* l3[3] = {s8 + 256 * p, s8 + 256 * (p == 2 ? 0 : p + 1), s8 + 256 * (p == 0 ? 2 : p - 1)};
                    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
                    for (int k = 0; k < 16; ++k) w[k >> 2] |= (uint32_t)l3[k % 3][chunk_byte(v[u], k)] << (8 * (k & 3));
                    v[u] = make_uint4(w[0], w[1], w[2], w[3]);
                }
                to[base + 256 * u] = v[u];
            }
    }
    if (blockIdx.x == 0) {
        if (tid < s.head) dst[tid] = on ? s8[256 * (tid % 3) + img[tid]] : img[tid];
        if (tid >= 16 && tid - 16 < s.tail) {
            const int64_t o = s.tail_at + (tid - 16);
            dst[o] = on ? s8[256 * (int)(o % 3) + img[o]] : img[o];
        }
    }
}

size_t tone_workspace_bytes(int B) { return align_up((size_t)B * TONE_HIST_BYTES, 256); }

// in -> out, (B, H, W, 3) u8, out == in allowed (no other overlap); ws: 16-byte aligned, tone_workspace_bytes() bytes = the histograms.
// Shapes and pointers are the caller's to check (B is a grid dimension: <= 65535; H W < 2^31).
int tone_stage(const uint8_t* in, uint8_t* out, void* ws, int B, int H, int W, const int* table, hipStream_t st) {
    uint32_t* hist = reinterpret_cast<uint32_t*>(ws);
    const int64_t n = (int64_t)H * W, nb = 3 * n;
    const int vec = ((reinterpret_cast<uintptr_t>(in) ^ reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
    const dim3 grid(std::max(1, cdiv(nb, TONE_STRIP_BYTES)), B);
    SD_HIP(hipMemsetAsync(hist, 0, (size_t)B * TONE_HIST_BYTES, st));
    hipLaunchKernelGGL(k_tone_hist, grid, dim3(TONE_HT), 0, st, in, hist, nb, table);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_tone_apply, grid, dim3(256), 0, st, in, out, hist, nb, table, vec);
    SD_LAUNCH_CHECK();
    return 0;
}

}  // namespace sd

using namespace sd;

extern "C" {

size_t sd_tone_workspace_bytes(int B) {
    if (B <= 0) return 0;
    return tone_workspace_bytes(B);
}

int sd_tone_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* table, void* workspace, size_t workspace_bytes,
               sd_stream_t stream) {
    SD_REQUIRE(in && out && table && workspace, SD_ERR_INVALID, "sd_tone_u8: null pointer");
    SD_REQUIRE(B > 0 && H > 0 && W > 0, SD_ERR_INVALID, "sd_tone_u8: bad shape");
    SD_REQUIRE(B <= 65535 && (int64_t)H * W < (1ll << 31), SD_ERR_INVALID, "sd_tone_u8: batch %d > 65535 or %d x %d >= 2^31 pixels", B, W, H);
    const int64_t bytes = (int64_t)B * H * W * 3;
    SD_REQUIRE(in == out || in + bytes <= out || out + bytes <= in, SD_ERR_INVALID, "sd_tone_u8: out must be in or not overlap it");
    SD_REQUIRE(aligned16(workspace), SD_ERR_INVALID, "sd_tone_u8: the workspace must be 16-byte aligned");
    SD_REQUIRE(workspace_bytes >= sd_tone_workspace_bytes(B), SD_ERR_WORKSPACE, "sd_tone_u8: workspace %zu < %zu", workspace_bytes,
               sd_tone_workspace_bytes(B));
    return tone_stage(in, out, workspace, B, H, W, table, (hipStream_t)stream);
}

}  // extern "C"
