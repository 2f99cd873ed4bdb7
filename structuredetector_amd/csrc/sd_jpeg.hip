// JPEG compression of 8-bit RGB images (`train --aug_jpeg`; not in the reference): byte for byte Pillow's Image.save(buf, "JPEG", quality=q)
// followed by Image.open(buf) = libjpeg-turbo, 4:2:0, accurate-integer DCT.  The entropy coder is lossless, so the round trip is
//     RGB -> YCbCr (jccolor) -> chroma h2v2 downsample (jcsample) -> forward DCT on sample - 128 (jfdctint: rows, then columns) -> quantise,
//     dequantise -> inverse DCT (jidctint: columns, then rows, range limit by mask) -> chroma h2v2 "fancy" upsample (jdsample) -> RGB (jdcolor)
// in signed 32-bit integers with arithmetic right shifts; tests/jpeg_ref.py states every formula and is pinned against Pillow.  The sides are
// multiples of 16 (whole MCUs).  table (B, 129) int32 on the device: [on, ql[64], qc[64]], the tables in natural order; on == 0 copies the
// image.  The table cannot be checked without a sync: entries are clamped to [1, 255] and none decides an address, so any table is safe.
//
// Two launches.  k_jpeg_code does everything up to the inverse DCT and writes the decoded Y plane at full size and the decoded Cb and Cr
// planes at half size (1.5 B/px) into the workspace; k_jpeg_rgb upsamples -- it needs the decoded chroma of the neighbouring MCUs, which one
// launch would have to recompute -- and converts.  The second launch reads the image only for a copy row, at the bytes it then writes, so
// out may be in.
//
// k_jpeg_code: a block of 256 threads owns a tile of 64 x 64 pixels = 4 x 4 MCUs, held in LDS as one sheet of 96 x 64 int32 samples,
// rows 0-63 luma, rows 64-95 chroma with Cb in columns 0-31 and Cr in columns 32-63: 96 blocks of 8 x 8, 768 eight-point transforms per
// pass, three per thread, each in registers.  The sheet's pitch is 65: a row pass has consecutive lanes on consecutive rows (bank = row mod
// 32), a column pass on consecutive columns, both conflict-free.  The forward column pass, the quantiser and the inverse column pass work on
// the same eight values, so a tile takes three transform phases: rows, columns (there and back), rows.  The sheet is the only tile-sized
// LDS buffer (26 KB a block, six blocks a CU): the RGB bytes come straight from global memory, 12 bytes = 4 pixels a lane and the 192 bytes
// of a tile row to 16 adjacent lanes (three dwords when the image is 4-byte aligned, else byte by byte), and the decoded bytes of an item go
// back into its own sheet words, from where the planes -- always aligned -- are written in 16-byte (Y) and 8-byte (Cb, Cr) chunks.
// k_jpeg_rgb writes 16 bytes at a time when the image is 16-byte aligned (3 W is a multiple of 16 here), else byte by byte.
#include "sd_common.h"

namespace sd {

constexpr int JT = 64;                                                   // tile side in pixels
constexpr int JS_ROWS = 96, JS_PITCH = 65;                               // the sample sheet
constexpr int JX = 16;                                                  // k_jpeg_rgb: output pixels of a thread in each of its two rows

constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373, F_1_175875602 = 9633;
constexpr int F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819, F_2_562915447 = 20995;
constexpr int F_3_072711026 = 25172;

__device__ __forceinline__ int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// the odd part both transforms share: (t4, t5, t6, t7) -> themselves as the four odd sums
__device__ __forceinline__ void dct_odd(int& t4, int& t5, int& t6, int& t7) {
    int z1 = t4 + t7, z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * F_1_175875602;
    t4 *= F_0_298631336; t5 *= F_2_053119869; t6 *= F_3_072711026; t7 *= F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447;
    z3 = z3 * -F_1_961570560 + z5; z4 = z4 * -F_0_390180644 + z5;
    t4 += z1 + z3; t5 += z2 + z4; t6 += z2 + z3; t7 += z1 + z4;
}

template <bool FIRST>
__device__ __forceinline__ void fdct8(int (&d)[8]) {
    constexpr int n = FIRST ? 11 : 15;
    const int t0 = d[0] + d[7], t1 = d[1] + d[6], t2 = d[2] + d[5], t3 = d[3] + d[4];
    int t7 = d[0] - d[7], t6 = d[1] - d[6], t5 = d[2] - d[5], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    d[0] = FIRST ? (t10 + t11) << 2 : descale(t10 + t11, 2);
    d[4] = FIRST ? (t10 - t11) << 2 : descale(t10 - t11, 2);
    const int z1 = (t12 + t13) * F_0_541196100;
    d[2] = descale(z1 + t13 * F_0_765366865, n);
    d[6] = descale(z1 - t12 * F_1_847759065, n);
    dct_odd(t4, t5, t6, t7);
    d[7] = descale(t4, n); d[5] = descale(t5, n); d[3] = descale(t6, n); d[1] = descale(t7, n);
}

template <bool FIRST>
__device__ __forceinline__ void idct8(int (&d)[8]) {
    constexpr int n = FIRST ? 11 : 18;
    const int z1 = (d[2] + d[6]) * F_0_541196100;
    const int t2 = z1 - d[6] * F_1_847759065, t3 = z1 + d[2] * F_0_765366865;
    const int t0 = (d[0] + d[4]) << 13, t1 = (d[0] - d[4]) << 13;
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    int a = d[7], b = d[5], c = d[3], e = d[1];
    dct_odd(a, b, c, e);
    d[0] = descale(t10 + e, n); d[7] = descale(t10 - e, n);
    d[1] = descale(t11 + c, n); d[6] = descale(t11 - c, n);
    d[2] = descale(t12 + b, n); d[5] = descale(t12 - b, n);
    d[3] = descale(t13 + a, n); d[4] = descale(t13 - a, n);
}

// jidctint's range_limit[x & RANGE_MASK]: the mask is the definition, not a clamp
__device__ __forceinline__ uint32_t range_limit(int x) {
    const int m = x & 1023;
    return (uint32_t)(m < 128 ? m + 128 : (m < 512 ? 255 : (m < 896 ? 0 : m - 896)));
}

__device__ __forceinline__ uint32_t byte12(uint32_t a0, uint32_t a1, uint32_t a2, int k) {
    return (((k >> 2) == 0 ? a0 : ((k >> 2) == 1 ? a1 : a2)) >> (8 * (k & 3))) & 255u;
}

// is the 8 x 8 block at sheet row r, column c inside the image?  nr x nc = the tile's pixels (multiples of 16)
__device__ __forceinline__ bool sheet_block_valid(int r, int c, int nr, int nc) {
    return r < JT ? (r < nr && c < nc) : (r - JT < (nr >> 1) && (c & 31) < (nc >> 1));
}

// in (B, H, W, 3) u8 -> plane_y (B, H, W), plane_cb, plane_cr (B, H / 2, W / 2) u8, decoded.  grid (cdiv(W, 64), cdiv(H, 64), B)
__global__ __launch_bounds__(256) void k_jpeg_code(const uint8_t* __restrict__ in, uint8_t* __restrict__ plane_y, uint8_t* __restrict__ plane_cb,
                                                    uint8_t* __restrict__ plane_cr, int H, int W, const int* __restrict__ table, int vec) {
    __shared__ int sheet[JS_ROWS * JS_PITCH];
    __shared__ int qt[128];                                             // ql, qc
    __shared__ uint32_t qm[128];                                         // their reciprocals (below)
    const int b = blockIdx.z, tid = threadIdx.x;
    const int* t = table + 129 * (int64_t)b;
    if (t[0] == 0) return;                                               // a copy row: k_jpeg_rgb copies (the whole block leaves)
    const int x0 = blockIdx.x * JT, y0 = blockIdx.y * JT;
    const int nr = min(JT, H - y0), nc = min(JT, W - x0);
    if (tid < 128) {
        // k = (n + q8 / 2) / q8 with q8 = 8 q in [8, 2040] as umulhi(n, m), m = floor((2^32 - 1) / q8) + 1.  Exact: m q8 = 2^32 + e with
        // 0 <= e < q8 (e = 0 when q8 is a power of two), so n m / 2^32 = n / q8 + n e / (q8 2^32), and with n = Q q8 + r, r <= q8 - 1, the
        // floor is Q whenever n e < 2^32.  n = |c| + q8 / 2 where |c| <= 8 * 1024 + rounding (64 samples of magnitude <= 128 against a basis
        // whose absolute sum is at most 8, output scaled by 8): n < 2^14, n e < 2^25.
        const int q = min(max(t[1 + tid], 1), 255);
        qt[tid] = q;
        qm[tid] = 0xffffffffu / (uint32_t)(8 * q) + 1u;
    }
    const int64_t rowb = (int64_t)W * 3;
    const uint8_t* src = in + ((int64_t)b * H + y0) * rowb + (int64_t)x0 * 3;
    // colour conversion and chroma downsampling straight from global memory: a thread takes 2 rows x 4 pixels = 2 x 12 bytes (three dwords
    // when the image is 4-byte aligned; the 16 lanes of a tile row read its 192 bytes), 8 luma samples and 2 samples of either chroma plane
    for (int idx = tid; idx < (JT / 2) * (JT / 4); idx += 256) {
        const int g = idx & 15, qy = idx >> 4;
        if (2 * qy >= nr || 4 * g >= nc) continue;
        int cb[2] = {0, 0}, cr[2] = {0, 0};
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const uint8_t* p = src + (2 * qy + dy) * rowb + 12 * g;
            uint32_t a0, a1, a2;
            if (vec) {
                a0 = reinterpret_cast<const uint32_t*>(p)[0]; a1 = reinterpret_cast<const uint32_t*>(p)[1]; a2 = reinterpret_cast<const uint32_t*>(p)[2];
            } else {
                a0 = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
                a1 = (uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24;
                a2 = (uint32_t)p[8] | (uint32_t)p[9] << 8 | (uint32_t)p[10] << 16 | (uint32_t)p[11] << 24;
            }
            int* y = sheet + (2 * qy + dy) * JS_PITCH + 4 * g;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int R = (int)byte12(a0, a1, a2, 3 * k), G = (int)byte12(a0, a1, a2, 3 * k + 1), B = (int)byte12(a0, a1, a2, 3 * k + 2);
                y[k] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
                cb[k >> 1] += (-11059 * R - 21709 * G + 32768 * B + 8388608 + 32767) >> 16;
                cr[k >> 1] += (32768 * R - 27439 * G - 5329 * B + 8388608 + 32767) >> 16;
            }
        }
        int* c = sheet + (JT + qy) * JS_PITCH + 2 * g;                   // the chroma column x0 / 2 + 2 g + j has the parity of j: bias 1, 2
        c[0] = ((cb[0] + 1) >> 2) - 128; c[1] = ((cb[1] + 2) >> 2) - 128;
        c[32] = ((cr[0] + 1) >> 2) - 128; c[33] = ((cr[1] + 2) >> 2) - 128;
    }
    __syncthreads();
    // forward DCT along the rows: lane -> sheet row
    for (int item = tid; item < JS_ROWS * 8; item += 256) {
        const int r = item % JS_ROWS, c0 = (item / JS_ROWS) * 8;
        if (!sheet_block_valid(r, c0, nr, nc)) continue;
        int* p = sheet + r * JS_PITCH + c0;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        fdct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k] = d[k];
    }
    __syncthreads();
    // forward DCT along the columns, quantise, dequantise, inverse DCT along the columns: lane -> sheet column
    for (int item = tid; item < (JS_ROWS / 8) * JT; item += 256) {
        const int c = item & (JT - 1), r0 = (item >> 6) * 8;
        if (!sheet_block_valid(r0, c, nr, nc)) continue;
        int* p = sheet + r0 * JS_PITCH + c;
        const int tb = (r0 < JT ? 0 : 64) + (c & 7);
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k * JS_PITCH];
        fdct8<false>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = qt[tb + 8 * k];
            const uint32_t n = (uint32_t)abs(d[k]) + (uint32_t)(4 * q);
            const int lv = (int)__umulhi(n, qm[tb + 8 * k]) * q;
            d[k] = d[k] < 0 ? -lv : lv;
        }
        idct8<true>(d);
#pragma unroll
        for (int k = 0; k < 8; ++k) p[k * JS_PITCH] = d[k];
    }
    __syncthreads();
    // inverse DCT along the rows and the range limit; the eight bytes go back into the first two of the item's own eight sheet words, for
    // whole-chunk stores below
    for (int item = tid; item < JS_ROWS * 8; item += 256) {
        const int r = item % JS_ROWS, c0 = (item / JS_ROWS) * 8;
        if (!sheet_block_valid(r, c0, nr, nc)) continue;
        int* p = sheet + r * JS_PITCH + c0;
        int d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) d[k] = p[k];
        idct8<false>(d);
        uint2 o;
        o.x = range_limit(d[0]) | range_limit(d[1]) << 8 | range_limit(d[2]) << 16 | range_limit(d[3]) << 24;
        o.y = range_limit(d[4]) | range_limit(d[5]) << 8 | range_limit(d[6]) << 16 | range_limit(d[7]) << 24;
        p[0] = (int)o.x; p[1] = (int)o.y;
    }
    __syncthreads();
    {                                                                    // luma: 64 rows x 4 chunks of 16 bytes = two items' words each
        const int row = tid >> 2, ch = tid & 3;
        if (row < nr && (ch << 4) < nc) {
            const int* s = sheet + row * JS_PITCH + (ch << 4);
            *reinterpret_cast<uint4*>(plane_y + ((int64_t)b * H + y0 + row) * W + x0 + (ch << 4)) =
                make_uint4((uint32_t)s[0], (uint32_t)s[1], (uint32_t)s[8], (uint32_t)s[9]);
        }
    }
    {                                                                    // chroma: 2 planes x 32 rows x 4 chunks of 8 bytes
        const int pl = tid >> 7, row = (tid >> 2) & 31, ch = tid & 3;
        if (row < (nr >> 1) && (ch << 3) < (nc >> 1)) {
            uint8_t* plane = pl ? plane_cr : plane_cb;
            const int Hc = H >> 1, Wc = W >> 1;
            const int* s = sheet + (JT + row) * JS_PITCH + 32 * pl + (ch << 3);
            *reinterpret_cast<uint2*>(plane + ((int64_t)b * Hc + (y0 >> 1) + row) * Wc + (x0 >> 1) + (ch << 3)) = make_uint2((uint32_t)s[0], (uint32_t)s[1]);
        }
    }
}

// a row of 8 decoded chroma samples with one sample on either side, clamped at the plane's edges: m[0 .. 9]
__device__ __forceinline__ void chroma_row(const uint8_t* __restrict__ row, int x8, int Wc, int (&m)[10]) {
    const uint2 v = *reinterpret_cast<const uint2*>(row + x8);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        m[1 + k] = (int)((v.x >> (8 * k)) & 255u);
        m[5 + k] = (int)((v.y >> (8 * k)) & 255u);
    }
    m[0] = x8 > 0 ? (int)row[x8 - 1] : m[1];
    m[9] = x8 + 8 < Wc ? (int)row[x8 + 8] : m[8];
}

// planes -> out (B, H, W, 3) u8; a copy row takes its bytes from in (which may be out).  One thread: 16 pixels of the output rows 2 y, 2 y + 1.
__global__ __launch_bounds__(256) void k_jpeg_rgb(const uint8_t* in, const uint8_t* __restrict__ plane_y, const uint8_t* __restrict__ plane_cb,
                                                   const uint8_t* __restrict__ plane_cr, uint8_t* out, int H, int W,
                                                   const int* __restrict__ table, int vec, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int nsx = W / JX, Hc = H >> 1, Wc = W >> 1;
    const int sx = (int)(idx % nsx);
    const int64_t rest = idx / nsx;
    const int y = (int)(rest % Hc);
    const int64_t b = rest / Hc;
    const int64_t rowb = (int64_t)W * 3;
    const int64_t at = (b * H + 2 * y) * rowb + (int64_t)sx * (JX * 3);
    if (table[129 * b] == 0) {
        if (in == out) return;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            const uint8_t* s = in + at + dy * rowb;
            uint8_t* d = out + at + dy * rowb;
            if (vec) {
#pragma unroll
                for (int k = 0; k < 3; ++k) reinterpret_cast<uint4*>(d)[k] = reinterpret_cast<const uint4*>(s)[k];
            } else {
                for (int k = 0; k < JX * 3; ++k) d[k] = s[k];
            }
        }
        return;
    }
    int cb[3][10], cr[3][10];                                            // rows y - 1, y, y + 1 (clamped)
    const int ys[3] = {max(y - 1, 0), y, min(y + 1, Hc - 1)};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t off = (b * Hc + ys[k]) * Wc;
        chroma_row(plane_cb + off, 8 * sx, Wc, cb[k]);
        chroma_row(plane_cr + off, 8 * sx, Wc, cr[k]);
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
        const uint4 yv = *reinterpret_cast<const uint4*>(plane_y + (b * H + 2 * y + dy) * W + JX * sx);
        const uint32_t yw[4] = {yv.x, yv.y, yv.z, yv.w};
        int sb[10], sr[10];                                              // 3 x the near row + the far one
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            sb[k] = 3 * cb[1][k] + cb[dy ? 2 : 0][k];
            sr[k] = 3 * cr[1][k] + cr[dy ? 2 : 0][k];
        }
        uint32_t w[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < JX; ++i) {
            const int j = 1 + (i >> 1);                                  // even pixel: the left neighbour and + 8; odd: the right one and + 7
            const int u = ((3 * sb[j] + ((i & 1) ? sb[j + 1] + 7 : sb[j - 1] + 8)) >> 4) - 128;
            const int v = ((3 * sr[j] + ((i & 1) ? sr[j + 1] + 7 : sr[j - 1] + 8)) >> 4) - 128;
            const int Y = (int)((yw[i >> 2] >> (8 * (i & 3))) & 255u);
            const uint32_t R = (uint32_t)min(max(Y + ((91881 * v + 32768) >> 16), 0), 255);
            const uint32_t G = (uint32_t)min(max(Y + ((-22554 * u + 32768 - 46802 * v) >> 16), 0), 255);
            const uint32_t B = (uint32_t)min(max(Y + ((116130 * u + 32768) >> 16), 0), 255);
            w[(3 * i) >> 2] |= R << (8 * ((3 * i) & 3));
            w[(3 * i + 1) >> 2] |= G << (8 * ((3 * i + 1) & 3));
            w[(3 * i + 2) >> 2] |= B << (8 * ((3 * i + 2) & 3));
        }
        uint8_t* d = out + at + dy * rowb;
        if (vec) {
#pragma unroll
            for (int k = 0; k < 3; ++k) reinterpret_cast<uint4*>(d)[k] = make_uint4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < JX * 3; ++k) d[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

size_t jpeg_planes_bytes(int B, int H, int W) { return align_up((size_t)B * H * W * 3 / 2, 256); }

// in -> planes -> out, in and out (B, H, W, 3) u8 with H and W multiples of 16, out == in allowed (no other overlap); planes: 16-byte
// aligned, jpeg_planes_bytes() bytes.  Shapes and pointers are the caller's to check.
int jpeg_stage(const uint8_t* in, uint8_t* out, uint8_t* planes, int B, int H, int W, const int* table, hipStream_t st) {
    const int vec = aligned16(in) && aligned16(out);
    const int dwords = (reinterpret_cast<uintptr_t>(in) & 3u) == 0;      // (3 W is a multiple of 4: every 4-pixel group is a dword triple then)
    uint8_t* py = planes;
    uint8_t* pcb = py + (size_t)B * H * W;
    uint8_t* pcr = pcb + (size_t)B * H * W / 4;
    hipLaunchKernelGGL(k_jpeg_code, dim3(cdiv(W, JT), cdiv(H, JT), B), dim3(256), 0, st, in, py, pcb, pcr, H, W, table, dwords);
    SD_LAUNCH_CHECK();
    const int64_t total = (int64_t)B * (H / 2) * (W / JX);
    hipLaunchKernelGGL(k_jpeg_rgb, dim3(cdiv(total, 256)), dim3(256), 0, st, in, py, pcb, pcr, out, H, W, table, vec, total);
    SD_LAUNCH_CHECK();
    return 0;
}

}  // namespace sd

using namespace sd;

extern "C" {

size_t sd_jpeg_workspace_bytes(int B, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0) return 0;
    return jpeg_planes_bytes(B, H, W);
}

int sd_jpeg_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* table, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_REQUIRE(in && out && table && workspace, SD_ERR_INVALID, "sd_jpeg_u8: null pointer");
    SD_REQUIRE(B > 0 && H > 0 && W > 0, SD_ERR_INVALID, "sd_jpeg_u8: bad shape");
    SD_REQUIRE(H % 16 == 0 && W % 16 == 0, SD_ERR_INVALID, "sd_jpeg_u8: %d x %d is not a whole number of 16 x 16 MCUs", W, H);
    SD_REQUIRE(B <= 65535 && H <= 65535 * JT && (int64_t)B * H * W * 3 < (1ll << 40), SD_ERR_INVALID, "sd_jpeg_u8: batch too large");
    const int64_t bytes = (int64_t)B * H * W * 3;
    SD_REQUIRE(in == out || in + bytes <= out || out + bytes <= in, SD_ERR_INVALID,
               "sd_jpeg_u8: out must be in or not overlap it");
    SD_REQUIRE(aligned16(workspace), SD_ERR_INVALID, "sd_jpeg_u8: the workspace must be 16-byte aligned");
    SD_REQUIRE(workspace_bytes >= sd_jpeg_workspace_bytes(B, H, W), SD_ERR_WORKSPACE, "sd_jpeg_u8: workspace %zu < %zu", workspace_bytes,
               sd_jpeg_workspace_bytes(B, H, W));
    return jpeg_stage(in, out, reinterpret_cast<uint8_t*>(workspace), B, H, W, table, (hipStream_t)stream);
}

}  // extern "C"
