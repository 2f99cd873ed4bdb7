// Gaussian blur of 8-bit RGB images (`train --aug_blur`; not in the reference): byte for byte Pillow's Image.filter(GaussianBlur(r)) =
// libImaging/BoxBlur.c, three box-blur passes along every row and then three along every column, every pass rounded to bytes, channels
// independent.  One pass over a line in[0 .. n-1] with c(i) = min(max(i, 0), n - 1):
//     out[x] = (ww * sum_{i = -R .. R} in[c(x + i)] + fw * (in[c(x - R - 1)] + in[c(x + R + 1)]) + 2^23) >> 24        (uint32)
// (R, ww, fw) per image come from the host (data/augment.py blur_box_params: float32 arithmetic restated from Pillow) in a device table
// blur (B, 3) int32; the device does integer work only.  The table cannot be checked without a sync: R is clamped to
// [0, SD_BLUR_MAX_RADIUS] and nothing else in a row decides an address, so any table is memory-safe.  A row with R == 0 and fw == 0 copies.
//
// Two launches, one per direction, each reading and writing the image once: a block stages a tile plus a halo of 3 (R + 1) positions on
// either side along the blur axis in LDS, runs the three passes there (ping-pong between two LDS buffers) and writes the tile.  The edge
// rule is replication of the pass's own INPUT line, so every pass indexes by c() in image coordinates: where the halo reaches the image
// border c() is the true clamp; where it does not, clamping to the staged extent only changes positions within (passes left) * (R + 1)
// of the extent's end, which lie in the halo and are never written.  The halo follows the image's own R (a copy row stages no halo).
// The walk along the blur axis keeps a running window sum -- S(x + 1) = S(x) + in[c(x + R + 1)] - in[c(x - R)], two LDS reads and one
// write per output whatever R is -- and a thread carries four byte lanes of one dword (their sums as 16-bit fields, 24-bit multiplies):
//   vertical   an LDS line is a piece of an image row (256 bytes: channels need no separating, the neighbour of a byte is the byte one
//              row down); a thread owns four adjacent byte columns and a segment of rows.
//   horizontal the tile is staged TRANSPOSED, LDS line = one channel of one pixel column (line 3 x + c), a line's bytes = the tile's 64
//              rows: the neighbour of a line is the line 3 further, a thread owns four adjacent image rows and a segment of columns, and
//              the same routine serves both directions.  The pitch of 68 bytes (17 dwords) spreads the 16-byte chunks of one image row,
//              which land 16 lines apart, over the banks.
// Global accesses are 16 bytes wide when 3 W is a multiple of 16 and the buffers are 16-byte aligned (every network input size is a
// multiple of 32), else byte by byte.
#include "sd_common.h"

namespace sd {

constexpr int BL_HALO = 3 * (SD_BLUR_MAX_RADIUS + 1);                    // positions a tile needs on either side at the largest R
constexpr int BL_ROWS = 64;                                              // image rows per tile, both kernels
constexpr int BH_PX = 80;                                                // horizontal: pixels per tile (240 bytes = 15 chunks of 16)
constexpr int BH_LINES = (BH_PX + 2 * BL_HALO) * 3, BH_PITCH = BL_ROWS + 4;
constexpr int BV_COLS = 256;                                             // vertical: byte columns per tile
constexpr int BV_LINES = BL_ROWS + 2 * BL_HALO, BV_PITCH = BV_COLS;

__device__ __forceinline__ int cdiv_dev(int a, int b) { return (a + b - 1) / b; }

struct BlurRow { int R; uint32_t ww, fw; bool copy; };

__device__ __forceinline__ BlurRow blur_row_of(const int* __restrict__ blur, int b) {
    const int* t = blur + 3 * (int64_t)b;
    const int R = min(max(t[0], 0), SD_BLUR_MAX_RADIUS);
    return BlurRow{R, (uint32_t)t[1], (uint32_t)t[2], R == 0 && t[2] == 0};
}

__device__ __forceinline__ uint32_t byte_of(const uint4& v, int j) {
    const uint32_t w = (j >> 2) == 0 ? v.x : ((j >> 2) == 1 ? v.y : ((j >> 2) == 2 ? v.z : v.w));
    return (w >> (8 * (j & 3))) & 255u;
}

// The three passes over a staged tile: position p in [0, E) and phase ph in [0, step) name LDS line p * step + ph, a line holds ndw
// dwords that matter.  Input in buf0, result in buf1; ends with a barrier.  All 256 threads call it.
__device__ __forceinline__ void blur_passes(uint8_t* buf0, uint8_t* buf1, int pitch, int ndw, int step, int E, const BlurRow& p) {
    const int lanes = ndw * step;
    const int nseg = max(1, min(256 / lanes, cdiv_dev(E, 8)));           // segments of the walk: at least 8 positions each
    const int seglen = cdiv_dev(E, nseg);
    const int ls = step * pitch;                                         // bytes from a position to the next
    const int R = p.R;
    const uint32_t ww = p.ww, fw = p.fw;
    uint8_t* src = buf0;
    uint8_t* dst = buf1;
    for (int pass = 0; pass < 3; ++pass) {
        for (int item = threadIdx.x; item < lanes * nseg; item += 256) {
            const int dw = item % ndw, ph = (item / ndw) % step, sg = item / lanes;
            const int p0 = sg * seglen, p1 = min(p0 + seglen, E);
            if (p0 >= p1) continue;
            const uint8_t* s = src + ph * pitch + dw * 4;
            uint8_t* d = dst + ph * pitch + dw * 4;
            auto ld = [&](int q) { return *reinterpret_cast<const uint32_t*>(s + min(max(q, 0), E - 1) * ls); };
            // byte lanes 0, 2 and 1, 3 as 16-bit fields of two dwords: a window sum is at most 15 * 255 and an edge pair 510, and
            // (sum + entering) - leaving never borrows across a field, the leaving byte being one of the window's.  The products are
            // 24 x 24 bits (ww < 2^24 whenever a row blurs: ww = 2^24 comes with R = 0, fw = 0, the copy row; fw <= 2^23).
            constexpr uint32_t M = 0x00ff00ffu;
            uint32_t sl = 0, sh = 0;
            for (int i = -R; i <= R; ++i) {
                const uint32_t v = ld(p0 + i);
                sl += v & M; sh += (v >> 8) & M;
            }
            uint32_t a = ld(p0 - R - 1);
            uint32_t al = a & M, ah = (a >> 8) & M;
            for (int q = p0; q < p1; ++q) {
                const uint32_t b = ld(q + R + 1);
                const uint32_t bl = b & M, bh = (b >> 8) & M;
                const uint32_t el = al + bl, eh = ah + bh;
                const uint32_t o0 = (__umul24(ww, sl & 0xffffu) + __umul24(fw, el & 0xffffu) + (1u << 23)) >> 24;
                const uint32_t o1 = (__umul24(ww, sh & 0xffffu) + __umul24(fw, eh & 0xffffu) + (1u << 23)) >> 24;
                const uint32_t o2 = (__umul24(ww, sl >> 16) + __umul24(fw, el >> 16) + (1u << 23)) >> 24;
                const uint32_t o3 = (__umul24(ww, sh >> 16) + __umul24(fw, eh >> 16) + (1u << 23)) >> 24;
                *reinterpret_cast<uint32_t*>(d + q * ls) = o0 | o1 << 8 | o2 << 16 | o3 << 24;
                a = ld(q - R);                                           // leaves the window, and is the next position's left edge pixel
                al = a & M; ah = (a >> 8) & M;
                sl = sl + bl - al; sh = sh + bh - ah;
            }
        }
        __syncthreads();
        uint8_t* t = src; src = dst; dst = t;
    }
}

// horizontal direction: in (B, H, W, 3) u8 -> out (B, H, W, 3) u8 (another buffer).  grid (cdiv(W, BH_PX), cdiv(H, BL_ROWS), B)
__global__ __launch_bounds__(256) void k_blur_h(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W,
                                                 const int* __restrict__ blur, int vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][BH_LINES * BH_PITCH];
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * BL_ROWS, nr = min(BL_ROWS, H - r0);
    const int t0 = blockIdx.x * BH_PX, t1 = min(t0 + BH_PX, W);
    const BlurRow p = blur_row_of(blur, b);
    const int halo = p.copy ? 0 : 3 * (p.R + 1);
    const int e0 = max(t0 - halo, 0), e1 = min(t1 + halo, W);            // staged pixel columns: at most BH_PX + 2 BL_HALO
    const int64_t rowb = (int64_t)W * 3;
    const uint8_t* src = in + ((int64_t)b * H + r0) * rowb;
    uint8_t* dst = out + ((int64_t)b * H + r0) * rowb;
    const int lo = e0 * 3, nb = (e1 - e0) * 3;                           // staged bytes of a row: [lo, lo + nb), LDS line = byte - lo
    uint8_t* l0 = lds[0];
    if (vec) {                                                           // 16 lanes on 16 rows, then the next chunk: 64 contiguous bytes per row
        const int c0 = lo >> 4, nch = ((lo + nb + 15) >> 4) - c0;      // (3 W is a multiple of 16: every chunk lies inside its row)
        for (int idx = threadIdx.x; idx < 16 * nch * ((nr + 15) >> 4); idx += 256) {
            const int rest = idx >> 4, ch = rest % nch, row = (rest / nch) * 16 + (idx & 15);
            if (row >= nr) continue;
            const uint4 v = *reinterpret_cast<const uint4*>(src + row * rowb + ((int64_t)(c0 + ch) << 4));
            const int base = ((c0 + ch) << 4) - lo;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (base + j >= 0 && base + j < nb) l0[(base + j) * BH_PITCH + row] = (uint8_t)byte_of(v, j);
        }
    } else {
        for (int idx = threadIdx.x; idx < nr * nb; idx += 256) {
            const int row = idx / nb, pos = idx - row * nb;
            l0[pos * BH_PITCH + row] = src[row * rowb + lo + pos];
        }
    }
    __syncthreads();
    if (!p.copy) blur_passes(lds[0], lds[1], BH_PITCH, (nr + 3) >> 2, 3, e1 - e0, p);
    const uint8_t* res = p.copy ? lds[0] : lds[1];
    const int o0 = t0 * 3 - lo, ob = (t1 - t0) * 3;                      // the tile's own bytes: lines [o0, o0 + ob)
    if (vec) {                                                           // t0 * 3 and ob are multiples of 16 here
        const int nch = ob >> 4;
        for (int idx = threadIdx.x; idx < 16 * nch * ((nr + 15) >> 4); idx += 256) {
            const int rest = idx >> 4, ch = rest % nch, row = (rest / nch) * 16 + (idx & 15);
            if (row >= nr) continue;
            const uint8_t* q = res + (o0 + (ch << 4)) * BH_PITCH + row;
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (uint32_t)q[(4 * k) * BH_PITCH] | (uint32_t)q[(4 * k + 1) * BH_PITCH] << 8 | (uint32_t)q[(4 * k + 2) * BH_PITCH] << 16 |
                       (uint32_t)q[(4 * k + 3) * BH_PITCH] << 24;
            *reinterpret_cast<uint4*>(dst + row * rowb + (int64_t)t0 * 3 + (ch << 4)) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    } else {
        for (int idx = threadIdx.x; idx < nr * ob; idx += 256) {
            const int row = idx / ob, pos = idx - row * ob;
            dst[row * rowb + (int64_t)t0 * 3 + pos] = res[(o0 + pos) * BH_PITCH + row];
        }
    }
}

// vertical direction: in (B, H, W, 3) u8 -> out (B, H, W, 3) u8 (another buffer).  grid (cdiv(3 W, BV_COLS), cdiv(H, BL_ROWS), B)
__global__ __launch_bounds__(256) void k_blur_v(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int H, int W,
                                                 const int* __restrict__ blur, int vec) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[2][BV_LINES * BV_PITCH];
    const int b = blockIdx.z;
    const int r0 = blockIdx.y * BL_ROWS, r1 = min(r0 + BL_ROWS, H);
    const int64_t rowb = (int64_t)W * 3;
    const int64_t c0 = (int64_t)blockIdx.x * BV_COLS;
    const int nc = (int)min((int64_t)BV_COLS, rowb - c0);
    const BlurRow p = blur_row_of(blur, b);
    const int halo = p.copy ? 0 : 3 * (p.R + 1);
    const int e0 = max(r0 - halo, 0), e1 = min(r1 + halo, H);            // staged rows: at most BL_ROWS + 2 BL_HALO
    const uint8_t* src = in + ((int64_t)b * H + e0) * rowb + c0;
    uint8_t* dst = out + ((int64_t)b * H + r0) * rowb + c0;
    uint8_t* l0 = lds[0];
    const int E = e1 - e0;
    if (vec) {                                                           // nc is a multiple of 16 here
        const int nch = nc >> 4;
        for (int idx = threadIdx.x; idx < E * nch; idx += 256) {
            const int line = idx / nch, ch = idx - line * nch;
            *reinterpret_cast<uint4*>(l0 + line * BV_PITCH + (ch << 4)) = *reinterpret_cast<const uint4*>(src + line * rowb + (ch << 4));
        }
    } else {
        for (int idx = threadIdx.x; idx < E * nc; idx += 256) {
            const int line = idx / nc, pos = idx - line * nc;
            l0[line * BV_PITCH + pos] = src[line * rowb + pos];
        }
    }
    __syncthreads();
    if (!p.copy) blur_passes(lds[0], lds[1], BV_PITCH, (nc + 3) >> 2, 1, E, p);
    const uint8_t* res = (p.copy ? lds[0] : lds[1]) + (r0 - e0) * BV_PITCH;
    const int nr = r1 - r0;
    if (vec) {
        const int nch = nc >> 4;
        for (int idx = threadIdx.x; idx < nr * nch; idx += 256) {
            const int line = idx / nch, ch = idx - line * nch;
            *reinterpret_cast<uint4*>(dst + line * rowb + (ch << 4)) = *reinterpret_cast<const uint4*>(res + line * BV_PITCH + (ch << 4));
        }
    } else {
        for (int idx = threadIdx.x; idx < nr * nc; idx += 256) {
            const int line = idx / nc, pos = idx - line * nc;
            dst[line * rowb + pos] = res[line * BV_PITCH + pos];
        }
    }
}

// both directions: in -> mid -> out, each (B, H, W, 3) u8; mid differs from in and out (out may be in).  Shapes are the caller's to check.
int blur_stage(const uint8_t* in, uint8_t* mid, uint8_t* out, int B, int H, int W, const int* blur, hipStream_t st) {
    const int vec = ((int64_t)W * 3) % 16 == 0 && aligned16(in) && aligned16(mid) && aligned16(out);
    hipLaunchKernelGGL(k_blur_h, dim3(cdiv(W, BH_PX), cdiv(H, BL_ROWS), B), dim3(256), 0, st, in, mid, H, W, blur, vec);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_blur_v, dim3(cdiv((int64_t)W * 3, BV_COLS), cdiv(H, BL_ROWS), B), dim3(256), 0, st, mid, out, H, W, blur, vec);
    SD_LAUNCH_CHECK();
    return 0;
}

}  // namespace sd

using namespace sd;

extern "C" {

size_t sd_blur_workspace_bytes(int B, int H, int W) { return align_up((size_t)B * H * W * 3, 256); }

int sd_blur_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* blur, void* workspace, size_t workspace_bytes,
               sd_stream_t stream) {
    SD_REQUIRE(in && out && blur && workspace, SD_ERR_INVALID, "sd_blur_u8: null pointer");
    SD_REQUIRE(in != out, SD_ERR_INVALID, "sd_blur_u8: in place is not supported (out must not overlap in)");
    SD_REQUIRE(B > 0 && H > 0 && W > 0, SD_ERR_INVALID, "sd_blur_u8: bad shape");
    SD_REQUIRE(B <= 65535 && H <= 65535 * BL_ROWS && (int64_t)B * H * W * 3 < (1ll << 40), SD_ERR_INVALID, "sd_blur_u8: batch too large");
    SD_REQUIRE(workspace_bytes >= sd_blur_workspace_bytes(B, H, W), SD_ERR_WORKSPACE, "sd_blur_u8: workspace %zu < %zu", workspace_bytes,
               sd_blur_workspace_bytes(B, H, W));
    return blur_stage(in, reinterpret_cast<uint8_t*>(workspace), out, B, H, W, blur, (hipStream_t)stream);
}

}  // extern "C"
