// Input pipeline on gfx950: resize + horizontal / vertical flip + ImageNet normalisation of a batch of
// decoded RGB images, replacing the PIL / torchvision chain the reference runs in its DataLoader workers
// (src/sdnet/data/transforms.py:9-35 flips, :47-60 Resize, :108-118 Normalize, composed at :217-234 and :255-261).
//
// Resize: torchvision's F.resize on a PIL image is PIL's Image.resize(BILINEAR) = a separable resampling with a triangle filter
// whose support grows with the scale factor (antialiased when shrinking), computed in 8-bit fixed point: horizontal pass into an
// 8-bit image, then the vertical pass (Pillow, src/libImaging/Resample.c: precompute_coeffs + normalize_coeffs_8bpc with
// PRECISION_BITS = 22, ImagingResampleHorizontal_8bpc / Vertical_8bpc; Pillow 12.2 is the dependency present in the image).
// The coefficient tables are computed on the host exactly like Pillow does (double -> 22-bit fixed point); the two kernels
// below reproduce the integer accumulation and the clip, so the resized bytes are IDENTICAL to PIL's -- which makes the
// normalised float image bit-identical to the reference's (to_tensor = u8 / 255 in fp32, then (x - mean) / std in fp32: two
// correctly rounded fp32 operations each; contraction is off in this file).
// HBM-bound byte work: reads B*Hin*Win*3, writes B*Hin*Wout*3 (8-bit intermediate) + B*3*Hout*Wout*4.
#pragma clang fp contract(off)
#include "sd_common.h"

namespace sd {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ uint8_t clip8(int v) {
    if (v >= (1 << PRECISION_BITS << 8)) return 255;
    if (v <= 0) return 0;
    return (uint8_t)(v >> PRECISION_BITS);
}

// horizontal pass: in (B, Hin, Win, 3) u8 -> tmp (B, Hin, Wout, 3) u8.  bounds[x] = {xmin, count}, kk[x * ksize + i] fixed-point weights
__global__ __launch_bounds__(256) void k_resample_h(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int Hin, int Win, int Wout,
                                                     const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int64_t rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one output pixel (3 bytes) per thread
    if (i >= rows * Wout) return;
    const int64_t row = i / Wout;
    const int x = (int)(i - row * Wout);
    const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
    const int* k = kk + (int64_t)x * ksize;
    const uint8_t* src = in + (row * Win + xmin) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t) {
        const int w = k[t];
        s0 += src[3 * t + 0] * w; s1 += src[3 * t + 1] * w; s2 += src[3 * t + 2] * w;
    }
    uint8_t* dst = out + i * 3;
    dst[0] = clip8(s0); dst[1] = clip8(s1); dst[2] = clip8(s2);
}

// horizontal pass from a device table of image pointers (sd_preprocess_images_list*): the bytes of k_resample_h, built for large
// sources read straight from HBM (a decoded-image cache).  A block owns `rpb` (<= HL_ROWS) consecutive source rows of one image -- rows of
// one image are contiguous -- and stages them into LDS with 16-byte global loads (the bytes before the first and after the last 16-byte
// boundary one by one: any byte offset works and nothing outside the image is read), then evaluates the taps from LDS, every thread
// owning output columns and reading each of its weights once for all the block's rows, four taps (12 bytes) at a time as four aligned
// dwords + v_alignbyte (integer sums: the order of the taps does not change a bit); the 8-bit intermediate is written row by row,
// consecutive threads on consecutive pixels.  Dynamic LDS: rpb * Win * 3 + 32 bytes (the offset mod 16 + the last window's overhang;
// bytes there are multiplied by zero weights).
constexpr int HL_ROWS = 4;
constexpr int HL_LDS_BYTES = 65536;
__global__ __launch_bounds__(256) void k_resample_h_list(const uint8_t* const* __restrict__ images, uint8_t* __restrict__ out, int Hin, int Win,
                                                          int Wout, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int rpb,
                                                          int blocks_per_image) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.x / blocks_per_image;
    const int r0 = (blockIdx.x - b * blocks_per_image) * rpb;
    const int nr = min(rpb, Hin - r0);
    const int L = Win * 3;                                               // row bytes (rpb * L + 32 <= HL_LDS_BYTES: checked by the host)
    const uint8_t* src = images[b] + (int64_t)r0 * L;
    const int span = nr * L;
    const int off = (int)(reinterpret_cast<uintptr_t>(src) & 15);      // LDS keeps the source's offset mod 16: 16-byte LDS stores stay aligned
    const int head = min((16 - off) & 15, span);
    const int nvec = (span - head) >> 4, tail = head + (nvec << 4);
    const uint4* vsrc = reinterpret_cast<const uint4*>(src + head);
    uint4* vdst = reinterpret_cast<uint4*>(lds + off + head);
    for (int base = 0; base < nvec; base += 8 * 256) {                  // 8 loads in flight per thread before the LDS stores
        uint4 v[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + k * 256 + threadIdx.x;
            v[k] = i < nvec ? vsrc[i] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int i = base + k * 256 + threadIdx.x;
            if (i < nvec) vdst[i] = v[k];
        }
    }
    if ((int)threadIdx.x < head) lds[off + threadIdx.x] = src[threadIdx.x];
    if ((int)threadIdx.x < span - tail) lds[off + tail + threadIdx.x] = src[tail + threadIdx.x];
    __syncthreads();
    for (int x = threadIdx.x; x < Wout; x += 256) {
        const int xmin = bounds[2 * x], n = bounds[2 * x + 1];
        const int* k = kk + (int64_t)x * ksize;
        int s[HL_ROWS][3];
#pragma unroll
        for (int r = 0; r < HL_ROWS; ++r) s[r][0] = s[r][1] = s[r][2] = 1 << (PRECISION_BITS - 1);
        for (int t0 = 0; t0 < n; t0 += 4) {                              // four taps = 12 source bytes per row: 4 dword LDS reads
            int w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = t0 + j < n ? k[t0 + j] : 0;
#pragma unroll
            for (int r = 0; r < HL_ROWS; ++r) {
                if (r < nr) {
                    const int q = off + r * L + (xmin + t0) * 3;           // first byte of the four pixels (reads stop 13 bytes past the rows)
                    const uint32_t* d = reinterpret_cast<const uint32_t*>(lds + (q & ~3));
                    const int sh = q & 3;
                    const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
                    const uint32_t a0 = __builtin_amdgcn_alignbyte(d1, d0, sh), a1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                                   a2 = __builtin_amdgcn_alignbyte(d3, d2, sh);   // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
                    s[r][0] += (int)(a0 & 255) * w[0] + (int)(a0 >> 24) * w[1] + (int)((a1 >> 16) & 255) * w[2] + (int)((a2 >> 8) & 255) * w[3];
                    s[r][1] += (int)((a0 >> 8) & 255) * w[0] + (int)(a1 & 255) * w[1] + (int)(a1 >> 24) * w[2] + (int)((a2 >> 16) & 255) * w[3];
                    s[r][2] += (int)((a0 >> 16) & 255) * w[0] + (int)((a1 >> 8) & 255) * w[1] + (int)(a2 & 255) * w[2] + (int)(a2 >> 24) * w[3];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < HL_ROWS; ++r) {
            if (r < nr) {
                uint8_t* dst = out + (((int64_t)b * Hin + r0 + r) * Wout + x) * 3;
                dst[0] = clip8(s[r][0]); dst[1] = clip8(s[r][1]); dst[2] = clip8(s[r][2]);
            }
        }
    }
}

// vertical pass + flips + to_tensor + Normalize: tmp (B, Hin, Wout, 3) u8 -> out (B, 3, Hout, Wout) fp32 NCHW
__global__ __launch_bounds__(256) void k_resample_v_norm(const uint8_t* __restrict__ in, float* __restrict__ out, int Hin, int Hout, int Wout,
                                                          const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                          const uint8_t* __restrict__ flips, float m0, float m1, float m2, float d0, float d1,
                                                          float d2, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one output pixel (three planes) per thread
    if (i >= (int64_t)B * Hout * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int y = (int)(t % Hout), b = (int)(t / Hout);
    const int f = flips ? flips[b] : 0;                                  // bit 0: horizontal flip, bit 1: vertical flip (applied AFTER the resize)
    const int sx = (f & 1) ? Wout - 1 - x : x, sy = (f & 2) ? Hout - 1 - y : y;
    const int ymin = bounds[2 * sy], n = bounds[2 * sy + 1];
    const int* k = kk + (int64_t)sy * ksize;
    const uint8_t* src = in + (((int64_t)b * Hin + ymin) * Wout + sx) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int r = 0; r < n; ++r) {
        const int w = k[r];
        const uint8_t* px = src + (int64_t)r * Wout * 3;
        s0 += px[0] * w; s1 += px[1] * w; s2 += px[2] * w;
    }
    const int64_t plane = (int64_t)Hout * Wout;
    float* o = out + (int64_t)b * 3 * plane + (int64_t)y * Wout + x;
    o[0] = ((float)clip8(s0) / 255.0f - m0) / d0;                        // to_tensor (u8 / 255), then Normalize: (x - mean) / std
    o[plane] = ((float)clip8(s1) / 255.0f - m1) / d1;
    o[2 * plane] = ((float)clip8(s2) / 255.0f - m2) / d2;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// RandomColorJitter (src/sdnet/data/transforms.py:37-47, in the default training chain :217-226) on the RESIZED 8-bit image, before the
// flips and Normalize: torchvision's ColorJitter on a PIL image = Pillow's ImageEnhance.Brightness / Contrast / Color and an HSV round
// trip for the hue, applied in a random order per image.  The byte arithmetic of Pillow (libImaging/Blend.c: float blend, truncated
// inside [0, 1], clipped outside; Convert.c: rgb2l, rgb2hsv_row, hsv2rgb with their float / double mix) is reproduced exactly --
// oracle/pil_photometric.py is the restatement pinned against Pillow over all 2^24 colours, this is the same arithmetic on the device
// (contraction is off in this file; float and double divisions are correctly rounded).
//   order word: bits 0-7 = the four op ids (2 bits each, first op in bits 0-1: 0 brightness, 1 contrast, 2 saturation, 3 hue),
//               bits 8-15 = the hue shift byte uint8(hue_factor * 255); factors = {brightness, contrast, saturation} as floats.
// Contrast blends with the image's mean grey level AT THAT POINT of the op order, a reduction over the whole image: k_jitter_lsum sums
// the grey level of every pixel after the ops that precede the contrast op (integer atomics: exact, order-independent).
// ---------------------------------------------------------------------------------------------------------------------------------
struct Rgb8 { int r, g, b; };

__device__ __forceinline__ int pil_l(const Rgb8& c) { return (c.r * 19595 + c.g * 38470 + c.b * 7471 + 0x8000) >> 16; }
__device__ __forceinline__ int pil_blend1(int d, int x, float a, bool inside) {
    const float t = (float)d + a * (float)(x - d);
    if (inside) return (int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}
__device__ __forceinline__ Rgb8 pil_blend(const Rgb8& d, const Rgb8& x, float a) {
    const bool inside = a >= 0.0f && a <= 1.0f;
    return Rgb8{pil_blend1(d.r, x.r, a, inside), pil_blend1(d.g, x.g, a, inside), pil_blend1(d.b, x.b, a, inside)};
}
__device__ __forceinline__ int clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ Rgb8 pil_hue(const Rgb8& c, int shift) {
    const int maxc = max(c.r, max(c.g, c.b)), minc = min(c.r, min(c.g, c.b));
    int uh = 0, us = 0;
    if (minc != maxc) {                                        // rgb2hsv_row
        const float cr = (float)(maxc - minc);
        const float sat = cr / (float)maxc;
        const float rc = (float)(maxc - c.r) / cr, gc = (float)(maxc - c.g) / cr, bc = (float)(maxc - c.b) / cr;
        float h;
        if (c.r == maxc) h = bc - gc;
        else if (c.g == maxc) h = (float)(2.0 + (double)rc - (double)bc);
        else h = (float)(4.0 + (double)gc - (double)rc);
        const double hd = (double)h / 6.0 + 1.0;
        h = (float)(hd - floor(hd));                           // fmod(x, 1.0) of a non-negative double
        uh = clip255((int)((double)h * 255.0));
        us = clip255((int)((double)sat * 255.0));
    }
    uh = (uh + shift) & 255;                                   // uint8 wrap-around (torchvision adjust_hue)
    if (us == 0) return Rgb8{maxc, maxc, maxc};                // hsv2rgb
    const double hf = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(hf);
    const float f = (float)(hf - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const double vf = (double)(float)maxc;
    const int p = clip255((int)floor(vf * (1.0 - (double)fs) + 0.5));
    const int q = clip255((int)floor(vf * (1.0 - (double)fs * (double)f) + 0.5));
    const int t = clip255((int)floor(vf * (1.0 - (double)fs * (1.0 - (double)f)) + 0.5));
    switch (i % 6) {
        case 0: return Rgb8{maxc, t, p};
        case 1: return Rgb8{q, maxc, p};
        case 2: return Rgb8{p, maxc, t};
        case 3: return Rgb8{p, q, maxc};
        case 4: return Rgb8{t, p, maxc};
        default: return Rgb8{maxc, p, q};
    }
}
// the ops of one image in order; stops BEFORE the contrast op when mean < 0 (the reduction pass)
__device__ __forceinline__ Rgb8 jitter_pixel(Rgb8 c, int order, float fb, float fc, float fs, int mean) {
    const int shift = (order >> 8) & 255;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int op = (order >> (2 * k)) & 3;
        if (op == 0) c = pil_blend(Rgb8{0, 0, 0}, c, fb);
        else if (op == 1) { if (mean < 0) return c; c = pil_blend(Rgb8{mean, mean, mean}, c, fc); }
        else if (op == 2) { const int l = pil_l(c); c = pil_blend(Rgb8{l, l, l}, c, fs); }
        else c = pil_hue(c, shift);
    }
    return c;
}

// vertical pass only: tmp (B, Hin, Wout, 3) u8 -> img (B, Hout, Wout, 3) u8 (the resized image the jitter works on)
__global__ __launch_bounds__(256) void k_resample_v_u8(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int Hin, int Hout, int Wout,
                                                        const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Hout * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int y = (int)(t % Hout), b = (int)(t / Hout);
    const int ymin = bounds[2 * y], n = bounds[2 * y + 1];
    const int* k = kk + (int64_t)y * ksize;
    const uint8_t* src = in + (((int64_t)b * Hin + ymin) * Wout + x) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int r = 0; r < n; ++r) {
        const int w = k[r];
        const uint8_t* px = src + (int64_t)r * Wout * 3;
        s0 += px[0] * w; s1 += px[1] * w; s2 += px[2] * w;
    }
    uint8_t* dst = out + i * 3;
    dst[0] = clip8(s0); dst[1] = clip8(s1); dst[2] = clip8(s2);
}

// grey-level sum of every image after the ops that precede its contrast op: blockIdx.y = image, grid-stride over its pixels
__global__ __launch_bounds__(256) void k_jitter_lsum(const uint8_t* __restrict__ img, int64_t npix, const int* __restrict__ order,
                                                      const float* __restrict__ factors, unsigned long long* __restrict__ lsum) {
    const int b = blockIdx.y;
    const int ord = order[b];
    const float fb = factors[3 * b], fc = factors[3 * b + 1], fs = factors[3 * b + 2];
    const uint8_t* src = img + (int64_t)b * npix * 3;
    unsigned long long acc = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const Rgb8 c = jitter_pixel(Rgb8{src[3 * i], src[3 * i + 1], src[3 * i + 2]}, ord, fb, fc, fs, -1);
        acc += (unsigned)pil_l(c);
    }
    acc = (unsigned long long)wave_sum((double)acc);           // < 2^53: exact in double
    if ((threadIdx.x & 63) == 0 && acc) atomicAdd(lsum + b, acc);
}

// jitter + flips + to_tensor + Normalize: img (B, Hout, Wout, 3) u8 -> out (B, 3, Hout, Wout) fp32 NCHW
__global__ __launch_bounds__(256) void k_jitter_norm(const uint8_t* __restrict__ img, float* __restrict__ out, int Hout, int Wout,
                                                      const int* __restrict__ order, const float* __restrict__ factors,
                                                      const unsigned long long* __restrict__ lsum, const uint8_t* __restrict__ flips, float m0,
                                                      float m1, float m2, float d0, float d1, float d2, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Hout * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int y = (int)(t % Hout), b = (int)(t / Hout);
    const int f = flips ? flips[b] : 0;
    const int sx = (f & 1) ? Wout - 1 - x : x, sy = (f & 2) ? Hout - 1 - y : y;
    const uint8_t* px = img + (((int64_t)b * Hout + sy) * Wout + sx) * 3;
    const int64_t plane = (int64_t)Hout * Wout;
    // ImageStat mean: exact sum / count in double, then int(mean + 0.5)
    const int mean = (int)((double)lsum[b] / (double)plane + 0.5);
    const Rgb8 c = jitter_pixel(Rgb8{px[0], px[1], px[2]}, order[b], factors[3 * b], factors[3 * b + 1], factors[3 * b + 2], mean);
    float* o = out + (int64_t)b * 3 * plane + (int64_t)y * Wout + x;
    o[0] = ((float)c.r / 255.0f - m0) / d0;
    o[plane] = ((float)c.g / 255.0f - m1) / d1;
    o[2 * plane] = ((float)c.b / 255.0f - m2) / d2;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// RandomAffine (rotate, scale, shift; no shear) on the RESIZED 8-bit image, in front of the jitter: torchvision's RandomAffine on a PIL
// image = Image.transform(size, AFFINE, inverse matrix, BILINEAR, fillcolor) = Pillow's generic transform (libImaging/Geometry.c:
// affine_transform + bilinear_filter32RGB), plain double arithmetic evaluated left to right and TRUNCATED to a byte -- a result one ulp
// below an integer changes the byte, so everything below is fp64 with contraction off (this file's pragma).  The host hands one inverse
// matrix (6 doubles, output pixel centre -> source position) per image; any finite matrix is legal, what maps outside the source is fill.
// A gather: a block owns a 64 x 16 tile of one image's output (a rotated footprint of about 64 x 64 source pixels at most: compact in L2),
// a thread four consecutive output pixels (whole-dword / 16-byte stores when the width is a multiple of 4).  The two horizontal neighbours
// of a tap are adjacent bytes: one 8-byte read per source row where three pixels remain in the row, byte reads at the right border.
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int AF_TX = 16, AF_TY = 16, AF_PX = 4;                         // threads per tile row, tile rows, pixels per thread

struct Affine6 { double m0, m1, m2, m3, m4, m5; };

__device__ __forceinline__ void affine_row(const uint8_t* __restrict__ row, int x0, int x1, bool wide, int* a, int* b) {
    if (wide) {                                                          // x1 == x0 + 1 and pixel x0 + 2 is in the row: 8 bytes stay inside it
        uint64_t v;
        __builtin_memcpy(&v, row + 3 * x0, 8);
        a[0] = (int)(v & 255); a[1] = (int)((v >> 8) & 255); a[2] = (int)((v >> 16) & 255);
        b[0] = (int)((v >> 24) & 255); b[1] = (int)((v >> 32) & 255); b[2] = (int)((v >> 40) & 255);
    } else {
        const uint8_t* p = row + 3 * x0;
        const uint8_t* q = row + 3 * x1;
        a[0] = p[0]; a[1] = p[1]; a[2] = p[2];
        b[0] = q[0]; b[1] = q[1]; b[2] = q[2];
    }
}

// the source position (xin, yin) of an (H, W, 3) image sampled as Pillow's bilinear_filter32RGB does; what lies outside is fill.  Shared
// by the affine and the projective form of the source-position arithmetic below.
__device__ __forceinline__ Rgb8 sample_bilinear(const uint8_t* __restrict__ src, int H, int W, double xin, double yin, const Rgb8& fill) {
    if (!(xin >= 0.0 && xin < (double)W && yin >= 0.0 && yin < (double)H)) return fill;       // (a NaN or an infinity is outside too)
    xin -= 0.5; yin -= 0.5;
    const double fx = floor(xin), fy = floor(yin);
    const double dx = xin - fx, dy = yin - fy;
    const int X = (int)fx, Y = (int)fy;                                  // -1 .. W - 1, -1 .. H - 1
    const int x0 = min(max(X, 0), W - 1), x1 = min(max(X + 1, 0), W - 1);
    const int y0 = min(max(Y, 0), H - 1), y1 = min(max(Y + 1, 0), H - 1);   // Y + 1 == H: Pillow sets v2 = v1, which row y0 read twice gives too
    const bool wide = X >= 0 && X + 2 < W;
    int a0[3], b0[3], a1[3], b1[3];
    affine_row(src + (int64_t)y0 * W * 3, x0, x1, wide, a0, b0);
    affine_row(src + (int64_t)y1 * W * 3, x0, x1, wide, a1, b1);
    int o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double v1 = (double)a0[c] + (double)(b0[c] - a0[c]) * dx;
        const double v2 = (double)a1[c] + (double)(b1[c] - a1[c]) * dx;
        o[c] = (int)(v1 + (v2 - v1) * dy) & 255;                         // (UINT8) of a value in [0, 255]
    }
    return Rgb8{o[0], o[1], o[2]};
}

// one output pixel (x, y): Pillow's affine_transform, then the sampling
__device__ __forceinline__ Rgb8 affine_pixel(const uint8_t* __restrict__ src, int H, int W, const Affine6& m, int x, int y, const Rgb8& fill) {
    const double xc = (double)x + 0.5, yc5 = (double)y + 0.5;
    const double xin = m.m0 * xc + m.m1 * yc5 + m.m2;
    const double yin = m.m3 * xc + m.m4 * yc5 + m.m5;
    return sample_bilinear(src, H, W, xin, yin, fill);
}

// Pillow's perspective_transform: both numerators divided by the same denominator, each quotient one correctly rounded fp64 division
// (a reciprocal and a multiply changes bytes).  den == 0 gives an infinity (fill) or, with a zero numerator, a NaN (fill here; undefined
// in Pillow); a negative den is sampled like any other where the position lands inside.
struct Persp8 { double a0, a1, a2, a3, a4, a5, a6, a7; };

__device__ __forceinline__ Rgb8 persp_pixel(const uint8_t* __restrict__ src, int H, int W, const Persp8& m, int x, int y, const Rgb8& fill) {
    const double xc = (double)x + 0.5, yc5 = (double)y + 0.5;
    const double den = m.a6 * xc + m.a7 * yc5 + 1.0;
    const double xin = (m.a0 * xc + m.a1 * yc5 + m.a2) / den;
    const double yin = (m.a3 * xc + m.a4 * yc5 + m.a5) / den;
    return sample_bilinear(src, H, W, xin, yin, fill);
}

__device__ __forceinline__ Affine6 affine_of(const double* __restrict__ affine, int b) {
    const double* m = affine + 6 * (int64_t)b;
    return Affine6{m[0], m[1], m[2], m[3], m[4], m[5]};
}

// img (B, H, W, 3) u8 -> out (B, H, W, 3) u8.  grid (cdiv(W, 64), cdiv(H, 16), B)
__global__ __launch_bounds__(256) void k_affine_u8(const uint8_t* __restrict__ img, uint8_t* __restrict__ out, int H, int W,
                                                    const double* __restrict__ affine, int f0, int f1, int f2) {
    const int b = blockIdx.z;
    const int x = (blockIdx.x * AF_TX + (threadIdx.x % AF_TX)) * AF_PX, y = blockIdx.y * AF_TY + threadIdx.x / AF_TX;
    if (x >= W || y >= H) return;
    const Affine6 m = affine_of(affine, b);
    const Rgb8 fill{f0, f1, f2};
    const uint8_t* src = img + (int64_t)b * H * W * 3;
    uint8_t* dst = out + (((int64_t)b * H + y) * W + x) * 3;
    if ((W & 3) == 0) {                                                  // four pixels = three aligned dwords
        Rgb8 c[AF_PX];
#pragma unroll
        for (int k = 0; k < AF_PX; ++k) c[k] = affine_pixel(src, H, W, m, x + k, y, fill);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        d[0] = (uint32_t)c[0].r | (uint32_t)c[0].g << 8 | (uint32_t)c[0].b << 16 | (uint32_t)c[1].r << 24;
        d[1] = (uint32_t)c[1].g | (uint32_t)c[1].b << 8 | (uint32_t)c[2].r << 16 | (uint32_t)c[2].g << 24;
        d[2] = (uint32_t)c[2].b | (uint32_t)c[3].r << 8 | (uint32_t)c[3].g << 16 | (uint32_t)c[3].b << 24;
    } else {
        for (int k = 0; k < AF_PX && x + k < W; ++k) {
            const Rgb8 c = affine_pixel(src, H, W, m, x + k, y, fill);
            dst[3 * k] = (uint8_t)c.r; dst[3 * k + 1] = (uint8_t)c.g; dst[3 * k + 2] = (uint8_t)c.b;
        }
    }
}

// RandomPerspective (`train --aug_perspective`): k_affine_u8 with the projective source position; persp (B, 8) fp64 on the device, the
// coefficients of Image.transform(size, PERSPECTIVE, ...).  Nothing in a row is validated: the inside test and the index clamps of
// sample_bilinear bound every address for any table.  img (B, H, W, 3) u8 -> out (B, H, W, 3) u8, never in place; k_affine_u8's grid.
__global__ __launch_bounds__(256) void k_persp_u8(const uint8_t* __restrict__ img, uint8_t* __restrict__ out, int H, int W,
                                                   const double* __restrict__ persp, int f0, int f1, int f2) {
    const int b = blockIdx.z;
    const int x = (blockIdx.x * AF_TX + (threadIdx.x % AF_TX)) * AF_PX, y = blockIdx.y * AF_TY + threadIdx.x / AF_TX;
    if (x >= W || y >= H) return;
    const double* a = persp + 8 * (int64_t)b;
    const Persp8 m{a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]};
    const Rgb8 fill{f0, f1, f2};
    const uint8_t* src = img + (int64_t)b * H * W * 3;
    uint8_t* dst = out + (((int64_t)b * H + y) * W + x) * 3;
    if ((W & 3) == 0) {                                                  // four pixels = three aligned dwords
        Rgb8 c[AF_PX];
#pragma unroll
        for (int k = 0; k < AF_PX; ++k) c[k] = persp_pixel(src, H, W, m, x + k, y, fill);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        d[0] = (uint32_t)c[0].r | (uint32_t)c[0].g << 8 | (uint32_t)c[0].b << 16 | (uint32_t)c[1].r << 24;
        d[1] = (uint32_t)c[1].g | (uint32_t)c[1].b << 8 | (uint32_t)c[2].r << 16 | (uint32_t)c[2].g << 24;
        d[2] = (uint32_t)c[2].b | (uint32_t)c[3].r << 8 | (uint32_t)c[3].g << 16 | (uint32_t)c[3].b << 24;
    } else {
        for (int k = 0; k < AF_PX && x + k < W; ++k) {
            const Rgb8 c = persp_pixel(src, H, W, m, x + k, y, fill);
            dst[3 * k] = (uint8_t)c.r; dst[3 * k + 1] = (uint8_t)c.g; dst[3 * k + 2] = (uint8_t)c.b;
        }
    }
}

// the same gather + flips + to_tensor + Normalize: img (B, H, W, 3) u8 -> out (B, 3, H, W) fp32 NCHW = k_affine_u8, then the flip and
// normalise arithmetic of k_resample_v_norm.  A thread owns four pixels of the WARPED image; a horizontal flip reverses them in the store.
__global__ __launch_bounds__(256) void k_affine_norm(const uint8_t* __restrict__ img, float* __restrict__ out, int H, int W,
                                                      const double* __restrict__ affine, int f0, int f1, int f2,
                                                      const uint8_t* __restrict__ flips, float m0, float m1, float m2, float d0, float d1,
                                                      float d2) {
    const int b = blockIdx.z;
    const int x = (blockIdx.x * AF_TX + (threadIdx.x % AF_TX)) * AF_PX, y = blockIdx.y * AF_TY + threadIdx.x / AF_TX;
    if (x >= W || y >= H) return;
    const Affine6 m = affine_of(affine, b);
    const Rgb8 fill{f0, f1, f2};
    const uint8_t* src = img + (int64_t)b * H * W * 3;
    const int f = flips ? flips[b] : 0;
    const int oy = (f & 2) ? H - 1 - y : y;
    const int64_t plane = (int64_t)H * W;
    float* o = out + (int64_t)b * 3 * plane + (int64_t)oy * W;
    if ((W & 3) == 0) {
        float r[AF_PX], g[AF_PX], bl[AF_PX];
#pragma unroll
        for (int k = 0; k < AF_PX; ++k) {
            const Rgb8 c = affine_pixel(src, H, W, m, x + k, y, fill);
            const int j = (f & 1) ? AF_PX - 1 - k : k;
            r[j] = ((float)c.r / 255.0f - m0) / d0;
            g[j] = ((float)c.g / 255.0f - m1) / d1;
            bl[j] = ((float)c.b / 255.0f - m2) / d2;
        }
        const int ox = (f & 1) ? W - AF_PX - x : x;
        *reinterpret_cast<float4*>(o + ox) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(o + plane + ox) = make_float4(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<float4*>(o + 2 * plane + ox) = make_float4(bl[0], bl[1], bl[2], bl[3]);
    } else {
        for (int k = 0; k < AF_PX && x + k < W; ++k) {
            const Rgb8 c = affine_pixel(src, H, W, m, x + k, y, fill);
            const int ox = (f & 1) ? W - 1 - (x + k) : x + k;
            o[ox] = ((float)c.r / 255.0f - m0) / d0;
            o[plane + ox] = ((float)c.g / 255.0f - m1) / d1;
            o[2 * plane + ox] = ((float)c.b / 255.0f - m2) / d2;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Mosaic (four images per sample) on the RESIZED 8-bit images, in front of the warp: the canvas of image b is cut at a centre (cx, cy)
// into four quadrants q = (x >= cx) + 2 (y >= cy), and quadrant q shows image s_q of the same batch under its own inverse matrix m_q --
// per pixel exactly Image.transform((W, H), AFFINE, m_q, BILINEAR, fillcolor) of resized[s_q] read at (x, y), i.e. affine_pixel on the
// canvas pixel centre.  geom (B, 6) int32 = cx, cy, s_0 .. s_3 and maffine (B, 4, 6) fp64 live on the device and cannot be checked by the
// host without a sync: cx, cy are clamped to [0, W], [0, H] and s_q to [0, B), so any table is memory-safe.  The launch shape of the
// affine kernels; a block whose 64 x 16 tile lies inside one quadrant (all but the one row and one column of blocks the centre cuts)
// loads its one matrix once and runs the affine kernels' loop, a straddling block selects source and matrix per pixel.  The sources are
// other images of the batch: never in place.
// ---------------------------------------------------------------------------------------------------------------------------------
struct MosaicGeom { int cx, cy, s0, s1, s2, s3; };

__device__ __forceinline__ MosaicGeom mosaic_geom_of(const int* __restrict__ geom, int b, int B, int H, int W) {
    const int* g = geom + 6 * (int64_t)b;
    return MosaicGeom{min(max(g[0], 0), W), min(max(g[1], 0), H), min(max(g[2], 0), B - 1), min(max(g[3], 0), B - 1),
                      min(max(g[4], 0), B - 1), min(max(g[5], 0), B - 1)};
}
__device__ __forceinline__ int mosaic_source(const MosaicGeom& g, int q) { return q == 0 ? g.s0 : (q == 1 ? g.s1 : (q == 2 ? g.s2 : g.s3)); }

// what a block needs to produce pixels: `uniform` = its whole tile lies in quadrant q0 (src / m are that quadrant's), else per pixel
struct MosaicTile {
    MosaicGeom g;
    bool uniform;
    const uint8_t* src;
    Affine6 m;
};

__device__ __forceinline__ MosaicTile mosaic_tile(const uint8_t* __restrict__ img, const int* __restrict__ geom,
                                                  const double* __restrict__ maffine, int b, int B, int H, int W) {
    MosaicTile t;
    t.g = mosaic_geom_of(geom, b, B, H, W);
    const int bx0 = blockIdx.x * AF_TX * AF_PX, by0 = blockIdx.y * AF_TY;
    t.uniform = (t.g.cx <= bx0 || t.g.cx >= bx0 + AF_TX * AF_PX) && (t.g.cy <= by0 || t.g.cy >= by0 + AF_TY);
    const int q0 = (bx0 >= t.g.cx ? 1 : 0) + (by0 >= t.g.cy ? 2 : 0);     // the quadrant of the tile's first pixel (the tile's, when uniform)
    t.src = img + (int64_t)mosaic_source(t.g, q0) * H * W * 3;
    t.m = affine_of(maffine, 4 * b + q0);
    return t;
}

__device__ __forceinline__ Rgb8 mosaic_pixel(const MosaicTile& t, const uint8_t* __restrict__ img, const double* __restrict__ maffine, int b,
                                             int H, int W, int x, int y, const Rgb8& fill) {
    if (t.uniform) return affine_pixel(t.src, H, W, t.m, x, y, fill);
    const int q = (x >= t.g.cx ? 1 : 0) + (y >= t.g.cy ? 2 : 0);
    return affine_pixel(img + (int64_t)mosaic_source(t.g, q) * H * W * 3, H, W, affine_of(maffine, 4 * b + q), x, y, fill);
}

// img (B, H, W, 3) u8 -> out (B, H, W, 3) u8 (another buffer).  grid (cdiv(W, 64), cdiv(H, 16), B)
__global__ __launch_bounds__(256) void k_mosaic_u8(const uint8_t* __restrict__ img, uint8_t* __restrict__ out, int H, int W,
                                                    const int* __restrict__ geom, const double* __restrict__ maffine, int f0, int f1, int f2) {
    const int b = blockIdx.z, B = gridDim.z;
    const int x = (blockIdx.x * AF_TX + (threadIdx.x % AF_TX)) * AF_PX, y = blockIdx.y * AF_TY + threadIdx.x / AF_TX;
    if (x >= W || y >= H) return;
    const MosaicTile t = mosaic_tile(img, geom, maffine, b, B, H, W);
    const Rgb8 fill{f0, f1, f2};
    uint8_t* dst = out + (((int64_t)b * H + y) * W + x) * 3;
    if ((W & 3) == 0) {                                                  // four pixels = three aligned dwords
        Rgb8 c[AF_PX];
#pragma unroll
        for (int k = 0; k < AF_PX; ++k) c[k] = mosaic_pixel(t, img, maffine, b, H, W, x + k, y, fill);
        uint32_t* d = reinterpret_cast<uint32_t*>(dst);
        d[0] = (uint32_t)c[0].r | (uint32_t)c[0].g << 8 | (uint32_t)c[0].b << 16 | (uint32_t)c[1].r << 24;
        d[1] = (uint32_t)c[1].g | (uint32_t)c[1].b << 8 | (uint32_t)c[2].r << 16 | (uint32_t)c[2].g << 24;
        d[2] = (uint32_t)c[2].b | (uint32_t)c[3].r << 8 | (uint32_t)c[3].g << 16 | (uint32_t)c[3].b << 24;
    } else {
        for (int k = 0; k < AF_PX && x + k < W; ++k) {
            const Rgb8 c = mosaic_pixel(t, img, maffine, b, H, W, x + k, y, fill);
            dst[3 * k] = (uint8_t)c.r; dst[3 * k + 1] = (uint8_t)c.g; dst[3 * k + 2] = (uint8_t)c.b;
        }
    }
}

// the same gather + flips + to_tensor + Normalize: img (B, H, W, 3) u8 -> out (B, 3, H, W) fp32 NCHW (the chain with neither warp nor jitter);
// the store of k_affine_norm
__global__ __launch_bounds__(256) void k_mosaic_norm(const uint8_t* __restrict__ img, float* __restrict__ out, int H, int W,
                                                      const int* __restrict__ geom, const double* __restrict__ maffine, int f0, int f1, int f2,
                                                      const uint8_t* __restrict__ flips, float m0, float m1, float m2, float d0, float d1,
                                                      float d2) {
    const int b = blockIdx.z, B = gridDim.z;
    const int x = (blockIdx.x * AF_TX + (threadIdx.x % AF_TX)) * AF_PX, y = blockIdx.y * AF_TY + threadIdx.x / AF_TX;
    if (x >= W || y >= H) return;
    const MosaicTile t = mosaic_tile(img, geom, maffine, b, B, H, W);
    const Rgb8 fill{f0, f1, f2};
    const int f = flips ? flips[b] : 0;
    const int oy = (f & 2) ? H - 1 - y : y;
    const int64_t plane = (int64_t)H * W;
    float* o = out + (int64_t)b * 3 * plane + (int64_t)oy * W;
    if ((W & 3) == 0) {
        float r[AF_PX], g[AF_PX], bl[AF_PX];
#pragma unroll
        for (int k = 0; k < AF_PX; ++k) {
            const Rgb8 c = mosaic_pixel(t, img, maffine, b, H, W, x + k, y, fill);
            const int j = (f & 1) ? AF_PX - 1 - k : k;
            r[j] = ((float)c.r / 255.0f - m0) / d0;
            g[j] = ((float)c.g / 255.0f - m1) / d1;
            bl[j] = ((float)c.b / 255.0f - m2) / d2;
        }
        const int ox = (f & 1) ? W - AF_PX - x : x;
        *reinterpret_cast<float4*>(o + ox) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(o + plane + ox) = make_float4(g[0], g[1], g[2], g[3]);
        *reinterpret_cast<float4*>(o + 2 * plane + ox) = make_float4(bl[0], bl[1], bl[2], bl[3]);
    } else {
        for (int k = 0; k < AF_PX && x + k < W; ++k) {
            const Rgb8 c = mosaic_pixel(t, img, maffine, b, H, W, x + k, y, fill);
            const int ox = (f & 1) ? W - 1 - (x + k) : x + k;
            o[ox] = ((float)c.r / 255.0f - m0) / d0;
            o[plane + ox] = ((float)c.g / 255.0f - m1) / d1;
            o[2 * plane + ox] = ((float)c.b / 255.0f - m2) / d2;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Windowed resize (crop training at the tile scale, `train --train_tiles`; not in the reference): image b's output is the Wout x Hout
// window at (x0_b, y0_b) of its resize to a Wc x Hc canvas -- byte for byte Image.resize((Wc, Hc), BILINEAR).crop((x0, y0, x0 + Wout,
// y0 + Hout)) -- without resampling the rest of the canvas: the tables are the canvas tables read at x0 + x and y0 + y, the horizontal
// pass covers only the source rows [rlo, rhi) under the window's rows (rlo = v_bounds[y0].first, rhi = v_bounds[y0 + Hout - 1].first +
// count) and the window's columns, and the intermediate is (B, max_rows, Wout, 3), image b's row r being source row rlo_b + r.
// window (B, 2) int32 = x0, y0 lives on the device and cannot be checked by the host without a sync: x0, y0 are clamped to [0, Wc - Wout],
// [0, Hc - Hout] and the row / column spans to the host's max_rows / max_cols, so any window table is memory-safe (the mosaic rule).
// ---------------------------------------------------------------------------------------------------------------------------------
struct Window { int x0, y0, rlo, nrows; };

__device__ __forceinline__ Window window_of(const int* __restrict__ window, const int* __restrict__ v_bounds, int b, int Hc, int Wc, int Hout,
                                            int Wout, int max_rows) {
    const int x0 = min(max(window[2 * b], 0), Wc - Wout), y0 = min(max(window[2 * b + 1], 0), Hc - Hout);
    const int last = y0 + Hout - 1;
    const int rlo = v_bounds[2 * y0], rhi = v_bounds[2 * last] + v_bounds[2 * last + 1];
    return Window{x0, y0, rlo, min(max(rhi - rlo, 1), max_rows)};
}

// horizontal pass, packed: in (B, Hin, Win, 3) u8 -> tmp (B, max_rows, Wout, 3) u8, one thread per intermediate pixel (k_resample_h's sum)
__global__ __launch_bounds__(256) void k_window_h(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int Hin, int Win, int Hc, int Wc,
                                                   int Hout, int Wout, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                   const int* __restrict__ v_bounds, const int* __restrict__ window, int max_rows, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * max_rows * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int r = (int)(t % max_rows), b = (int)(t / max_rows);
    const Window wd = window_of(window, v_bounds, b, Hc, Wc, Hout, Wout, max_rows);
    if (r >= wd.nrows) return;                                           // rows past this window's span are never read
    const int cx = wd.x0 + x;
    const int xmin = bounds[2 * cx], n = bounds[2 * cx + 1];
    const int* k = kk + (int64_t)cx * ksize;
    const uint8_t* src = in + (((int64_t)b * Hin + wd.rlo + r) * Win + xmin) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int t = 0; t < n; ++t) {
        const int w = k[t];
        s0 += src[3 * t + 0] * w; s1 += src[3 * t + 1] * w; s2 += src[3 * t + 2] * w;
    }
    uint8_t* dst = out + i * 3;
    dst[0] = clip8(s0); dst[1] = clip8(s1); dst[2] = clip8(s2);
}

// horizontal pass from a device table of image pointers: the block shape and the tap loop of k_resample_h_list -- a block owns `rpb`
// (<= HL_ROWS) consecutive rows of one window's span -- but it stages only the bytes of source columns [clo, chi) of each row (clo =
// bounds[x0].first, chi = bounds[x0 + Wout - 1].first + count).  Those pieces are not contiguous in memory: every row is staged on its
// own, with 16-byte global loads between its first and last 16-byte boundary and byte loads outside them (any byte offset works and
// nothing outside the image is read).  In LDS the rows lie S = 3 ncols + (0 .. 3) bytes apart, S = the source pitch mod 4, the first at the
// source's offset mod 4: every row keeps its address mod 4, so a 16-byte load is stored as four aligned dwords.  Dynamic LDS: rpb *
// max_cols * 3 + 32 bytes (offset <= 3, pitch padding <= 9, the last tap group's overhang 13; bytes there are multiplied by zero weights).
__global__ __launch_bounds__(256) void k_window_h_list(const uint8_t* const* __restrict__ images, uint8_t* __restrict__ out, int Win, int Hc, int Wc,
                                                        int Hout, int Wout, const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                        const int* __restrict__ v_bounds, const int* __restrict__ window, int max_rows,
                                                        int max_cols, int rpb, int blocks_per_image) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.x / blocks_per_image;
    const int r0 = (blockIdx.x - b * blocks_per_image) * rpb;
    const Window wd = window_of(window, v_bounds, b, Hc, Wc, Hout, Wout, max_rows);
    const int nr = min(rpb, wd.nrows - r0);
    if (nr <= 0) return;                                                 // (the whole block: nobody waits at the barrier)
    const int lastc = wd.x0 + Wout - 1;
    const int clo = bounds[2 * wd.x0];
    const int ncols = min(max(bounds[2 * lastc] + bounds[2 * lastc + 1] - clo, 1), max_cols);
    const int L = ncols * 3;                                             // staged bytes per row (rpb * L + 32 <= HL_LDS_BYTES: checked by the host)
    const int64_t pitch = (int64_t)Win * 3;
    const uint8_t* src0 = images[b] + ((int64_t)(wd.rlo + r0) * Win + clo) * 3;
    const int off = (int)(reinterpret_cast<uintptr_t>(src0) & 3);
    const int S = L + (int)((pitch - L) & 3);
    const uint8_t* rs[HL_ROWS];
    int hd[HL_ROWS], nv[HL_ROWS], maxv = 0;
#pragma unroll
    for (int r = 0; r < HL_ROWS; ++r) {
        rs[r] = src0 + (int64_t)min(r, nr - 1) * pitch;
        hd[r] = min((16 - (int)(reinterpret_cast<uintptr_t>(rs[r]) & 15)) & 15, L);
        nv[r] = r < nr ? (L - hd[r]) >> 4 : 0;
        maxv = max(maxv, nv[r]);
    }
    for (int base = 0; base < maxv; base += 2 * 256) {                  // up to 8 loads in flight per thread before the LDS stores
        uint4 v[HL_ROWS][2];
#pragma unroll
        for (int r = 0; r < HL_ROWS; ++r) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = base + k * 256 + threadIdx.x;
                v[r][k] = i < nv[r] ? reinterpret_cast<const uint4*>(rs[r] + hd[r])[i] : make_uint4(0, 0, 0, 0);
            }
        }
#pragma unroll
        for (int r = 0; r < HL_ROWS; ++r) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int i = base + k * 256 + threadIdx.x;
                if (i < nv[r]) {
                    uint32_t* d = reinterpret_cast<uint32_t*>(lds + off + r * S + hd[r]) + 4 * i;
                    d[0] = v[r][k].x; d[1] = v[r][k].y; d[2] = v[r][k].z; d[3] = v[r][k].w;
                }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < HL_ROWS; ++r) {
        if (r < nr) {
            const int tail = hd[r] + (nv[r] << 4);
            if ((int)threadIdx.x < hd[r]) lds[off + r * S + threadIdx.x] = rs[r][threadIdx.x];
            if ((int)threadIdx.x < L - tail) lds[off + r * S + tail + threadIdx.x] = rs[r][tail + threadIdx.x];
        }
    }
    __syncthreads();
    for (int x = threadIdx.x; x < Wout; x += 256) {
        const int cx = wd.x0 + x;
        const int xmin = bounds[2 * cx] - clo, n = bounds[2 * cx + 1];
        const int* k = kk + (int64_t)cx * ksize;
        int s[HL_ROWS][3];
#pragma unroll
        for (int r = 0; r < HL_ROWS; ++r) s[r][0] = s[r][1] = s[r][2] = 1 << (PRECISION_BITS - 1);
        for (int t0 = 0; t0 < n; t0 += 4) {
            int w[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) w[j] = t0 + j < n ? k[t0 + j] : 0;
            const int p = min(max(xmin + t0, 0), ncols - 1);           // a staged column whatever the tables say (inside already when they agree)
#pragma unroll
            for (int r = 0; r < HL_ROWS; ++r) {
                if (r < nr) {
                    const int q = off + r * S + p * 3;                   // first byte of the four pixels (reads stop 13 bytes past the row)
                    const uint32_t* d = reinterpret_cast<const uint32_t*>(lds + (q & ~3));
                    const int sh = q & 3;
                    const uint32_t d0 = d[0], d1 = d[1], d2 = d[2], d3 = d[3];
                    const uint32_t a0 = __builtin_amdgcn_alignbyte(d1, d0, sh), a1 = __builtin_amdgcn_alignbyte(d2, d1, sh),
                                   a2 = __builtin_amdgcn_alignbyte(d3, d2, sh);   // bytes r0 g0 b0 r1 | g1 b1 r2 g2 | b2 r3 g3 b3
                    s[r][0] += (int)(a0 & 255) * w[0] + (int)(a0 >> 24) * w[1] + (int)((a1 >> 16) & 255) * w[2] + (int)((a2 >> 8) & 255) * w[3];
                    s[r][1] += (int)((a0 >> 8) & 255) * w[0] + (int)(a1 & 255) * w[1] + (int)(a1 >> 24) * w[2] + (int)((a2 >> 16) & 255) * w[3];
                    s[r][2] += (int)((a0 >> 16) & 255) * w[0] + (int)((a1 >> 8) & 255) * w[1] + (int)(a2 & 255) * w[2] + (int)(a2 >> 24) * w[3];
                }
            }
        }
#pragma unroll
        for (int r = 0; r < HL_ROWS; ++r) {
            if (r < nr) {
                uint8_t* dst = out + (((int64_t)b * max_rows + r0 + r) * Wout + x) * 3;
                dst[0] = clip8(s[r][0]); dst[1] = clip8(s[r][1]); dst[2] = clip8(s[r][2]);
            }
        }
    }
}

// one output pixel of the vertical pass on a window: table row y0 + y, intermediate rows relative to rlo (kept inside the span)
__device__ __forceinline__ Rgb8 window_v_pixel(const uint8_t* __restrict__ in, int Wout, const int* __restrict__ bounds, const int* __restrict__ kk,
                                               int ksize, const Window& wd, int max_rows, int b, int x, int y) {
    const int ty = wd.y0 + y;
    const int ymin = bounds[2 * ty] - wd.rlo, n = bounds[2 * ty + 1];
    const int* k = kk + (int64_t)ty * ksize;
    const uint8_t* src = in + ((int64_t)b * max_rows * Wout + x) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int r = 0; r < n; ++r) {
        const int w = k[r];
        const uint8_t* px = src + (int64_t)min(max(ymin + r, 0), wd.nrows - 1) * Wout * 3;
        s0 += px[0] * w; s1 += px[1] * w; s2 += px[2] * w;
    }
    return Rgb8{clip8(s0), clip8(s1), clip8(s2)};
}

// vertical pass + flips + to_tensor + Normalize on a window: tmp (B, max_rows, Wout, 3) u8 -> out (B, 3, Hout, Wout) fp32 NCHW (k_resample_v_norm)
__global__ __launch_bounds__(256) void k_window_v_norm(const uint8_t* __restrict__ in, float* __restrict__ out, int Hc, int Wc, int Hout, int Wout,
                                                        const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                        const int* __restrict__ window, int max_rows, const uint8_t* __restrict__ flips, float m0,
                                                        float m1, float m2, float d0, float d1, float d2, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Hout * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int y = (int)(t % Hout), b = (int)(t / Hout);
    const int f = flips ? flips[b] : 0;                                  // the flips act on the WINDOW, after the resize
    const int sx = (f & 1) ? Wout - 1 - x : x, sy = (f & 2) ? Hout - 1 - y : y;
    const Window wd = window_of(window, bounds, b, Hc, Wc, Hout, Wout, max_rows);
    const Rgb8 c = window_v_pixel(in, Wout, bounds, kk, ksize, wd, max_rows, b, sx, sy);
    const int64_t plane = (int64_t)Hout * Wout;
    float* o = out + (int64_t)b * 3 * plane + (int64_t)y * Wout + x;
    o[0] = ((float)c.r / 255.0f - m0) / d0;
    o[plane] = ((float)c.g / 255.0f - m1) / d1;
    o[2 * plane] = ((float)c.b / 255.0f - m2) / d2;
}

// vertical pass only on a window: tmp (B, max_rows, Wout, 3) u8 -> img (B, Hout, Wout, 3) u8, what the mosaic / warp / jitter stages work on
__global__ __launch_bounds__(256) void k_window_v_u8(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int Hc, int Wc, int Hout, int Wout,
                                                      const int* __restrict__ bounds, const int* __restrict__ kk, int ksize,
                                                      const int* __restrict__ window, int max_rows, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Hout * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int y = (int)(t % Hout), b = (int)(t / Hout);
    const Window wd = window_of(window, bounds, b, Hc, Wc, Hout, Wout, max_rows);
    const Rgb8 c = window_v_pixel(in, Wout, bounds, kk, ksize, wd, max_rows, b, x, y);
    uint8_t* dst = out + i * 3;
    dst[0] = (uint8_t)c.r; dst[1] = (uint8_t)c.g; dst[2] = (uint8_t)c.b;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Letterbox (`--keep_aspect`; not in the reference): the Resize targets the largest Wi x Hi of the source's aspect ratio that fits the
// Wout x Hout frame (data/augment.py letterbox_geometry) and the resized image is pasted at (x0, y0) into a frame of fill3 -- byte for
// byte Image.new("RGB", (Wout, Hout), fill).paste(Image.resize((Wi, Hi), BILINEAR), (x0, y0)).  The horizontal pass is the plain one at
// Wout = Wi (k_resample_h / k_resample_h_list); the vertical pass below produces the frame, one thread per FRAME pixel: inside the
// placed rectangle k_resample_v_*'s sum on table row y - y0 and intermediate column x - x0, outside it the fill colour -- a bar pixel
// reads neither the tables nor the intermediate.  The geometry is uniform over the batch (batches are grouped by source size) and
// checked by the host half: host integers, no table, no clamp.
// ---------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ Rgb8 letterbox_pixel(const uint8_t* __restrict__ in, int Hin, int Hi, int Wi, int y0, int x0,
                                                const int* __restrict__ bounds, const int* __restrict__ kk, int ksize, int b, int x, int y,
                                                const Rgb8& fill) {
    const int ix = x - x0, iy = y - y0;
    if (ix < 0 || ix >= Wi || iy < 0 || iy >= Hi) return fill;
    const int ymin = bounds[2 * iy], n = bounds[2 * iy + 1];
    const int* k = kk + (int64_t)iy * ksize;
    const uint8_t* src = in + (((int64_t)b * Hin + ymin) * Wi + ix) * 3;
    int s0 = 1 << (PRECISION_BITS - 1), s1 = s0, s2 = s0;
    for (int r = 0; r < n; ++r) {
        const int w = k[r];
        const uint8_t* px = src + (int64_t)r * Wi * 3;
        s0 += px[0] * w; s1 += px[1] * w; s2 += px[2] * w;
    }
    return Rgb8{clip8(s0), clip8(s1), clip8(s2)};
}

// vertical pass + paste + flips + to_tensor + Normalize: tmp (B, Hin, Wi, 3) u8 -> out (B, 3, Hout, Wout) fp32 NCHW.  The flips act on the
// FRAME; a bar pixel goes through the same float expressions as an image pixel (bit-identical to normalising a fill byte).
__global__ __launch_bounds__(256) void k_letterbox_v_norm(const uint8_t* __restrict__ in, float* __restrict__ out, int Hin, int Hi, int Wi, int Hout,
                                                           int Wout, int y0, int x0, const int* __restrict__ bounds, const int* __restrict__ kk,
                                                           int ksize, const uint8_t* __restrict__ flips, int f0, int f1, int f2, float m0, float m1,
                                                           float m2, float d0, float d1, float d2, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;          // one frame pixel (three planes) per thread
    if (i >= (int64_t)B * Hout * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int y = (int)(t % Hout), b = (int)(t / Hout);
    const int f = flips ? flips[b] : 0;
    const int sx = (f & 1) ? Wout - 1 - x : x, sy = (f & 2) ? Hout - 1 - y : y;
    const Rgb8 c = letterbox_pixel(in, Hin, Hi, Wi, y0, x0, bounds, kk, ksize, b, sx, sy, Rgb8{f0, f1, f2});
    const int64_t plane = (int64_t)Hout * Wout;
    float* o = out + (int64_t)b * 3 * plane + (int64_t)y * Wout + x;
    o[0] = ((float)c.r / 255.0f - m0) / d0;
    o[plane] = ((float)c.g / 255.0f - m1) / d1;
    o[2 * plane] = ((float)c.b / 255.0f - m2) / d2;
}

// vertical pass + paste only: tmp (B, Hin, Wi, 3) u8 -> img (B, Hout, Wout, 3) u8, the frame the mosaic / warp / jitter stages work on
__global__ __launch_bounds__(256) void k_letterbox_v_u8(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int Hin, int Hi, int Wi, int Hout,
                                                         int Wout, int y0, int x0, const int* __restrict__ bounds, const int* __restrict__ kk,
                                                         int ksize, int f0, int f1, int f2, int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Hout * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int y = (int)(t % Hout), b = (int)(t / Hout);
    const Rgb8 c = letterbox_pixel(in, Hin, Hi, Wi, y0, x0, bounds, kk, ksize, b, x, y, Rgb8{f0, f1, f2});
    uint8_t* dst = out + i * 3;
    dst[0] = (uint8_t)c.r; dst[1] = (uint8_t)c.g; dst[2] = (uint8_t)c.b;
}

// flips + to_tensor + Normalize of an 8-bit image: img (B, Hout, Wout, 3) u8 -> out (B, 3, Hout, Wout) fp32 NCHW.  The tail of the blur forms
// without jitter (k_jitter_norm with neutral factors is not the identity on bytes: its float blends truncate); the expressions of
// k_resample_v_norm on the byte.
__global__ __launch_bounds__(256) void k_u8_norm(const uint8_t* __restrict__ img, float* __restrict__ out, int Hout, int Wout,
                                                  const uint8_t* __restrict__ flips, float m0, float m1, float m2, float d0, float d1, float d2,
                                                  int B) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)B * Hout * Wout) return;
    const int x = (int)(i % Wout);
    const int64_t t = i / Wout;
    const int y = (int)(t % Hout), b = (int)(t / Hout);
    const int f = flips ? flips[b] : 0;
    const int sx = (f & 1) ? Wout - 1 - x : x, sy = (f & 2) ? Hout - 1 - y : y;
    const uint8_t* px = img + (((int64_t)b * Hout + sy) * Wout + sx) * 3;
    const int64_t plane = (int64_t)Hout * Wout;
    float* o = out + (int64_t)b * 3 * plane + (int64_t)y * Wout + x;
    o[0] = ((float)px[0] / 255.0f - m0) / d0;
    o[plane] = ((float)px[1] / 255.0f - m1) / d1;
    o[2 * plane] = ((float)px[2] / 255.0f - m2) / d2;
}

}  // namespace sd

using namespace sd;

extern "C" {

size_t sd_preprocess_workspace_bytes(int B, int Hin, int Win, int Wout) { return align_up((size_t)B * Hin * Wout * 3, 256); }

size_t sd_preprocess_jitter_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout) {
    return sd_preprocess_workspace_bytes(B, Hin, Win, Wout) + align_up((size_t)B * Hout * Wout * 3, 256) + align_up((size_t)B * 8, 256);
}

static int preprocess_check(const char* what, const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                            int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const float* mean3, const float* std3, float* out,
                            void* workspace) {
    SD_REQUIRE(images && out && h_bounds && h_kk && v_bounds && v_kk && mean3 && std3 && workspace, SD_ERR_INVALID, "%s: null pointer", what);
    SD_REQUIRE(B > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0 && h_ksize > 0 && v_ksize > 0, SD_ERR_INVALID, "%s: bad shape", what);
    SD_REQUIRE((int64_t)B * std::max(Hin, Hout) * std::max(Win, Wout) * 3 < (1ll << 40), SD_ERR_INVALID, "%s: batch too large", what);
    SD_REQUIRE(std3[0] != 0.f && std3[1] != 0.f && std3[2] != 0.f, SD_ERR_INVALID, "%s: zero std", what);
    return 0;
}

// the launches after the horizontal pass (tmp = its 8-bit intermediate at the start of the workspace), shared by the packed and the list forms
static int preprocess_tail(int B, int Hin, int Hout, int Wout, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                           const float* mean3, const float* std3, float* out, uint8_t* tmp, hipStream_t st) {
    hipLaunchKernelGGL(k_resample_v_norm, dim3(cdiv((int64_t)B * Hout * Wout, 256)), dim3(256), 0, st, tmp, out, Hin, Hout, Wout, v_bounds, v_kk,
                       v_ksize, flips, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], B);
    SD_LAUNCH_CHECK();
    return 0;
}

// vertical pass into an 8-bit image, and the two jitter launches on an 8-bit image: the halves of the jitter tail, shared with the affine forms
static int resample_v_u8(int B, int Hin, int Hout, int Wout, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* tmp, uint8_t* img,
                         hipStream_t st) {
    hipLaunchKernelGGL(k_resample_v_u8, dim3(cdiv((int64_t)B * Hout * Wout, 256)), dim3(256), 0, st, tmp, img, Hin, Hout, Wout, v_bounds, v_kk,
                       v_ksize, B);
    SD_LAUNCH_CHECK();
    return 0;
}

static int jitter_norm(int B, int Hout, int Wout, const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const float* mean3,
                       const float* std3, float* out, const uint8_t* img, unsigned long long* lsum, hipStream_t st) {
    const int64_t npix = (int64_t)Hout * Wout;
    hipLaunchKernelGGL(k_jitter_lsum, dim3(std::min<int64_t>(cdiv(npix, 256), 64), B), dim3(256), 0, st, img, npix, jitter_order, jitter_factors, lsum);
    SD_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_jitter_norm, dim3(cdiv((int64_t)B * npix, 256)), dim3(256), 0, st, img, out, Hout, Wout, jitter_order, jitter_factors, lsum,
                       flips, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], B);
    SD_LAUNCH_CHECK();
    return 0;
}

static int preprocess_jitter_tail(int B, int Hin, int Win, int Hout, int Wout, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                  const int* jitter_order, const float* jitter_factors, const float* mean3, const float* std3, float* out,
                                  uint8_t* tmp, hipStream_t st) {
    uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
    unsigned long long* lsum = reinterpret_cast<unsigned long long*>(img + align_up((size_t)B * Hout * Wout * 3, 256));
    if (int e = resample_v_u8(B, Hin, Hout, Wout, v_bounds, v_kk, v_ksize, tmp, img, st)) return e;
    return jitter_norm(B, Hout, Wout, flips, jitter_order, jitter_factors, mean3, std3, out, img, lsum, st);
}

int sd_preprocess_images(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                         int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const float* mean3,
                         const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    if (int e = preprocess_check("sd_preprocess_images", images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, mean3, std3,
                                 out, workspace)) return e;
    SD_REQUIRE(workspace_bytes >= sd_preprocess_workspace_bytes(B, Hin, Win, Wout), SD_ERR_WORKSPACE, "sd_preprocess_images: workspace %zu < %zu",
               workspace_bytes, sd_preprocess_workspace_bytes(B, Hin, Win, Wout));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    const int64_t rows = (int64_t)B * Hin;
    hipLaunchKernelGGL(k_resample_h, dim3(cdiv(rows * Wout, 256)), dim3(256), 0, st, images, tmp, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rows);
    SD_LAUNCH_CHECK();
    return preprocess_tail(B, Hin, Hout, Wout, v_bounds, v_kk, v_ksize, flips, mean3, std3, out, tmp, st);
}

int sd_preprocess_images_jitter(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const float* mean3, const float* std3, float* out, void* workspace,
                                size_t workspace_bytes, sd_stream_t stream) {
    if (int e = preprocess_check("sd_preprocess_images_jitter", images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, mean3,
                                 std3, out, workspace)) return e;
    SD_REQUIRE(jitter_order && jitter_factors, SD_ERR_INVALID, "sd_preprocess_images_jitter: null jitter parameters");
    SD_REQUIRE(B <= 65535, SD_ERR_INVALID, "sd_preprocess_images_jitter: batch %d > 65535", B);
    SD_REQUIRE(workspace_bytes >= sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout), SD_ERR_WORKSPACE,
               "sd_preprocess_images_jitter: workspace %zu < %zu", workspace_bytes, sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
    SD_HIP(hipMemsetAsync(img + align_up((size_t)B * Hout * Wout * 3, 256), 0, (size_t)B * 8, st));        // lsum
    const int64_t rows = (int64_t)B * Hin;
    hipLaunchKernelGGL(k_resample_h, dim3(cdiv(rows * Wout, 256)), dim3(256), 0, st, images, tmp, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rows);
    SD_LAUNCH_CHECK();
    return preprocess_jitter_tail(B, Hin, Win, Hout, Wout, v_bounds, v_kk, v_ksize, flips, jitter_order, jitter_factors, mean3, std3, out, tmp, st);
}

// ---- the same from a device table of B image pointers (k_resample_h_list for the horizontal pass) ----
static int preprocess_list_check(const char* what, const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds,
                                 const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const float* mean3,
                                 const float* std3, float* out, void* workspace, int* rpb, int* blocks_per_image) {
    if (int e = preprocess_check(what, reinterpret_cast<const uint8_t*>(images), B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                 v_ksize, mean3, std3, out, workspace)) return e;
    SD_REQUIRE((int64_t)Win * 3 + 32 <= HL_LDS_BYTES, SD_ERR_INVALID, "%s: source rows of %d pixels exceed the LDS staging buffer (at most %d)",
               what, Win, (HL_LDS_BYTES - 32) / 3);
    *rpb = (int)std::min<int64_t>(HL_ROWS, (HL_LDS_BYTES - 32) / ((int64_t)Win * 3));
    *blocks_per_image = cdiv(Hin, *rpb);
    SD_REQUIRE((int64_t)B * *blocks_per_image < (1ll << 31), SD_ERR_INVALID, "%s: batch too large", what);
    return 0;
}

static int resample_h_list(const uint8_t* const* images, uint8_t* tmp, int B, int Hin, int Win, int Wout, const int* h_bounds, const int* h_kk,
                           int h_ksize, int rpb, int blocks_per_image, hipStream_t st) {
    const size_t lds = (size_t)rpb * Win * 3 + 32;
    hipLaunchKernelGGL(k_resample_h_list, dim3((unsigned)((int64_t)B * blocks_per_image)), dim3(256), lds, st, images, tmp, Hin, Win, Wout, h_bounds,
                       h_kk, h_ksize, rpb, blocks_per_image);
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_preprocess_images_list(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                              int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const float* mean3,
                              const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    int rpb = 0, bpi = 0;
    if (int e = preprocess_list_check("sd_preprocess_images_list", images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                                      mean3, std3, out, workspace, &rpb, &bpi)) return e;
    SD_REQUIRE(workspace_bytes >= sd_preprocess_workspace_bytes(B, Hin, Win, Wout), SD_ERR_WORKSPACE, "sd_preprocess_images_list: workspace %zu < %zu",
               workspace_bytes, sd_preprocess_workspace_bytes(B, Hin, Win, Wout));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (int e = resample_h_list(images, tmp, B, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rpb, bpi, st)) return e;
    return preprocess_tail(B, Hin, Hout, Wout, v_bounds, v_kk, v_ksize, flips, mean3, std3, out, tmp, st);
}

int sd_preprocess_images_list_jitter(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                     int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                     const float* jitter_factors, const float* mean3, const float* std3, float* out, void* workspace,
                                     size_t workspace_bytes, sd_stream_t stream) {
    int rpb = 0, bpi = 0;
    if (int e = preprocess_list_check("sd_preprocess_images_list_jitter", images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                      v_ksize, mean3, std3, out, workspace, &rpb, &bpi)) return e;
    SD_REQUIRE(jitter_order && jitter_factors, SD_ERR_INVALID, "sd_preprocess_images_list_jitter: null jitter parameters");
    SD_REQUIRE(B <= 65535, SD_ERR_INVALID, "sd_preprocess_images_list_jitter: batch %d > 65535", B);
    SD_REQUIRE(workspace_bytes >= sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout), SD_ERR_WORKSPACE,
               "sd_preprocess_images_list_jitter: workspace %zu < %zu", workspace_bytes, sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout));
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
    SD_HIP(hipMemsetAsync(img + align_up((size_t)B * Hout * Wout * 3, 256), 0, (size_t)B * 8, st));        // lsum
    if (int e = resample_h_list(images, tmp, B, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rpb, bpi, st)) return e;
    return preprocess_jitter_tail(B, Hin, Win, Hout, Wout, v_bounds, v_kk, v_ksize, flips, jitter_order, jitter_factors, mean3, std3, out, tmp, st);
}

// ---- RandomAffine between the resize and the jitter / normalise (k_affine_u8, k_affine_norm) ----
// workspace: the jitter forms' [horizontal intermediate | 8-bit image | grey sums] + a second 8-bit image.  The vertical pass writes the
// second image, the warp reads it: with jitter into the first (where the jitter launches expect their input), without straight to `out`.
size_t sd_preprocess_affine_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout) {
    return sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout) + align_up((size_t)B * Hout * Wout * 3, 256);
}

static int affine_check(const char* what, int B, int Hin, int Win, int Hout, int Wout, const int* jitter_order, const float* jitter_factors,
                        const double* affine, const uint8_t* fill3, size_t workspace_bytes) {
    SD_REQUIRE(affine && fill3, SD_ERR_INVALID, "%s: null affine matrices or fill colour", what);
    SD_REQUIRE((jitter_order == nullptr) == (jitter_factors == nullptr), SD_ERR_INVALID,
               "%s: jitter_order and jitter_factors go together (both null = no jitter)", what);
    SD_REQUIRE(B <= 65535, SD_ERR_INVALID, "%s: batch %d > 65535", what, B);
    SD_REQUIRE(workspace_bytes >= sd_preprocess_affine_workspace_bytes(B, Hin, Win, Hout, Wout), SD_ERR_WORKSPACE, "%s: workspace %zu < %zu", what,
               workspace_bytes, sd_preprocess_affine_workspace_bytes(B, Hin, Win, Hout, Wout));
    return 0;
}

// the launches after the vertical pass (`resized` = the 8-bit resized image), shared with the window forms
static int affine_stages(int B, int Hout, int Wout, const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                         const uint8_t* fill3, const float* mean3, const float* std3, float* out, const uint8_t* resized, uint8_t* img,
                         unsigned long long* lsum, hipStream_t st) {
    const dim3 grid(cdiv(Wout, AF_TX * AF_PX), cdiv(Hout, AF_TY), B);
    if (!jitter_order) {
        hipLaunchKernelGGL(k_affine_norm, grid, dim3(256), 0, st, resized, out, Hout, Wout, affine, (int)fill3[0], (int)fill3[1], (int)fill3[2], flips,
                           mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]);
        SD_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(k_affine_u8, grid, dim3(256), 0, st, resized, img, Hout, Wout, affine, (int)fill3[0], (int)fill3[1], (int)fill3[2]);
    SD_LAUNCH_CHECK();
    return jitter_norm(B, Hout, Wout, flips, jitter_order, jitter_factors, mean3, std3, out, img, lsum, st);
}

// the launches after the horizontal pass
static int preprocess_affine_tail(int B, int Hin, int Win, int Hout, int Wout, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                  const int* jitter_order, const float* jitter_factors, const double* affine, const uint8_t* fill3,
                                  const float* mean3, const float* std3, float* out, uint8_t* tmp, hipStream_t st) {
    uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
    unsigned long long* lsum = reinterpret_cast<unsigned long long*>(img + align_up((size_t)B * Hout * Wout * 3, 256));
    uint8_t* resized = tmp + sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout);
    if (int e = resample_v_u8(B, Hin, Hout, Wout, v_bounds, v_kk, v_ksize, tmp, resized, st)) return e;
    return affine_stages(B, Hout, Wout, flips, jitter_order, jitter_factors, affine, fill3, mean3, std3, out, resized, img, lsum, st);
}

int sd_preprocess_images_affine(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const double* affine, const uint8_t* fill3, const float* mean3, const float* std3,
                                float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    if (int e = preprocess_check("sd_preprocess_images_affine", images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, mean3,
                                 std3, out, workspace)) return e;
    if (int e = affine_check("sd_preprocess_images_affine", B, Hin, Win, Hout, Wout, jitter_order, jitter_factors, affine, fill3, workspace_bytes))
        return e;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (jitter_order) {
        uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
        SD_HIP(hipMemsetAsync(img + align_up((size_t)B * Hout * Wout * 3, 256), 0, (size_t)B * 8, st));    // lsum
    }
    const int64_t rows = (int64_t)B * Hin;
    hipLaunchKernelGGL(k_resample_h, dim3(cdiv(rows * Wout, 256)), dim3(256), 0, st, images, tmp, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rows);
    SD_LAUNCH_CHECK();
    return preprocess_affine_tail(B, Hin, Win, Hout, Wout, v_bounds, v_kk, v_ksize, flips, jitter_order, jitter_factors, affine, fill3, mean3, std3,
                                  out, tmp, st);
}

int sd_preprocess_images_list_affine(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                     const int* jitter_order, const float* jitter_factors, const double* affine, const uint8_t* fill3,
                                     const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                     sd_stream_t stream) {
    int rpb = 0, bpi = 0;
    if (int e = preprocess_list_check("sd_preprocess_images_list_affine", images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                      v_ksize, mean3, std3, out, workspace, &rpb, &bpi)) return e;
    if (int e = affine_check("sd_preprocess_images_list_affine", B, Hin, Win, Hout, Wout, jitter_order, jitter_factors, affine, fill3,
                             workspace_bytes)) return e;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (jitter_order) {
        uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
        SD_HIP(hipMemsetAsync(img + align_up((size_t)B * Hout * Wout * 3, 256), 0, (size_t)B * 8, st));    // lsum
    }
    if (int e = resample_h_list(images, tmp, B, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rpb, bpi, st)) return e;
    return preprocess_affine_tail(B, Hin, Win, Hout, Wout, v_bounds, v_kk, v_ksize, flips, jitter_order, jitter_factors, affine, fill3, mean3, std3,
                                  out, tmp, st);
}

// ---- Mosaic between the resize and the warp / jitter / normalise (k_mosaic_u8, k_mosaic_norm) ----
// workspace: that of the affine forms, [horizontal intermediate | 8-bit image A | grey sums | 8-bit image B].  The jitter launches read A, so
// the 8-bit stages are laid out backwards from there: without a warp the vertical pass writes B and the mosaic A (or `out`, fused); with a
// warp the vertical pass writes A, the mosaic B, and the warp A again (or `out`, fused) -- A's resized bytes are dead by then.
size_t sd_preprocess_mosaic_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout) {
    return sd_preprocess_affine_workspace_bytes(B, Hin, Win, Hout, Wout);
}

static int mosaic_check(const char* what, int B, int Hin, int Win, int Hout, int Wout, const int* jitter_order, const float* jitter_factors,
                        const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3, size_t workspace_bytes) {
    SD_REQUIRE(mosaic_geom && mosaic_affine && fill3, SD_ERR_INVALID, "%s: null mosaic tables or fill colour", what);
    SD_REQUIRE((jitter_order == nullptr) == (jitter_factors == nullptr), SD_ERR_INVALID,
               "%s: jitter_order and jitter_factors go together (both null = no jitter)", what);
    SD_REQUIRE(B <= 65535, SD_ERR_INVALID, "%s: batch %d > 65535", what, B);
    SD_REQUIRE(workspace_bytes >= sd_preprocess_mosaic_workspace_bytes(B, Hin, Win, Hout, Wout), SD_ERR_WORKSPACE, "%s: workspace %zu < %zu", what,
               workspace_bytes, sd_preprocess_mosaic_workspace_bytes(B, Hin, Win, Hout, Wout));
    return 0;
}

// the launches after the vertical pass, shared with the window forms: the resized image is in A with a warp, in B without (see above)
static int mosaic_stages(int B, int Hout, int Wout, const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                         const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                         uint8_t* img_a, uint8_t* img_b, unsigned long long* lsum, hipStream_t st) {
    uint8_t* resized = affine ? img_a : img_b;
    uint8_t* mosaic = affine ? img_b : img_a;
    const int f0 = fill3[0], f1 = fill3[1], f2 = fill3[2];
    const dim3 grid(cdiv(Wout, AF_TX * AF_PX), cdiv(Hout, AF_TY), B);
    if (!affine && !jitter_order) {
        hipLaunchKernelGGL(k_mosaic_norm, grid, dim3(256), 0, st, resized, out, Hout, Wout, mosaic_geom, mosaic_affine, f0, f1, f2, flips, mean3[0],
                           mean3[1], mean3[2], std3[0], std3[1], std3[2]);
        SD_LAUNCH_CHECK();
        return 0;
    }
    hipLaunchKernelGGL(k_mosaic_u8, grid, dim3(256), 0, st, resized, mosaic, Hout, Wout, mosaic_geom, mosaic_affine, f0, f1, f2);
    SD_LAUNCH_CHECK();
    if (affine && !jitter_order) {
        hipLaunchKernelGGL(k_affine_norm, grid, dim3(256), 0, st, mosaic, out, Hout, Wout, affine, f0, f1, f2, flips, mean3[0], mean3[1], mean3[2],
                           std3[0], std3[1], std3[2]);
        SD_LAUNCH_CHECK();
        return 0;
    }
    if (affine) {
        hipLaunchKernelGGL(k_affine_u8, grid, dim3(256), 0, st, mosaic, img_a, Hout, Wout, affine, f0, f1, f2);
        SD_LAUNCH_CHECK();
    }
    return jitter_norm(B, Hout, Wout, flips, jitter_order, jitter_factors, mean3, std3, out, img_a, lsum, st);
}

// the launches after the horizontal pass
static int preprocess_mosaic_tail(int B, int Hin, int Win, int Hout, int Wout, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                  const int* jitter_order, const float* jitter_factors, const double* affine, const int* mosaic_geom,
                                  const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                                  uint8_t* tmp, hipStream_t st) {
    uint8_t* img_a = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
    unsigned long long* lsum = reinterpret_cast<unsigned long long*>(img_a + align_up((size_t)B * Hout * Wout * 3, 256));
    uint8_t* img_b = tmp + sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout);
    if (int e = resample_v_u8(B, Hin, Hout, Wout, v_bounds, v_kk, v_ksize, tmp, affine ? img_a : img_b, st)) return e;
    return mosaic_stages(B, Hout, Wout, flips, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, img_a, img_b,
                         lsum, st);
}

int sd_preprocess_images_mosaic(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const double* affine, const int* mosaic_geom, const double* mosaic_affine,
                                const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                sd_stream_t stream) {
    if (int e = preprocess_check("sd_preprocess_images_mosaic", images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, mean3,
                                 std3, out, workspace)) return e;
    if (int e = mosaic_check("sd_preprocess_images_mosaic", B, Hin, Win, Hout, Wout, jitter_order, jitter_factors, mosaic_geom, mosaic_affine, fill3,
                             workspace_bytes)) return e;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (jitter_order) {
        uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
        SD_HIP(hipMemsetAsync(img + align_up((size_t)B * Hout * Wout * 3, 256), 0, (size_t)B * 8, st));    // lsum
    }
    const int64_t rows = (int64_t)B * Hin;
    hipLaunchKernelGGL(k_resample_h, dim3(cdiv(rows * Wout, 256)), dim3(256), 0, st, images, tmp, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rows);
    SD_LAUNCH_CHECK();
    return preprocess_mosaic_tail(B, Hin, Win, Hout, Wout, v_bounds, v_kk, v_ksize, flips, jitter_order, jitter_factors, affine, mosaic_geom,
                                  mosaic_affine, fill3, mean3, std3, out, tmp, st);
}

int sd_preprocess_images_list_mosaic(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                     const int* jitter_order, const float* jitter_factors, const double* affine, const int* mosaic_geom,
                                     const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                                     void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    int rpb = 0, bpi = 0;
    if (int e = preprocess_list_check("sd_preprocess_images_list_mosaic", images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                      v_ksize, mean3, std3, out, workspace, &rpb, &bpi)) return e;
    if (int e = mosaic_check("sd_preprocess_images_list_mosaic", B, Hin, Win, Hout, Wout, jitter_order, jitter_factors, mosaic_geom, mosaic_affine,
                             fill3, workspace_bytes)) return e;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (jitter_order) {
        uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
        SD_HIP(hipMemsetAsync(img + align_up((size_t)B * Hout * Wout * 3, 256), 0, (size_t)B * 8, st));    // lsum
    }
    if (int e = resample_h_list(images, tmp, B, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rpb, bpi, st)) return e;
    return preprocess_mosaic_tail(B, Hin, Win, Hout, Wout, v_bounds, v_kk, v_ksize, flips, jitter_order, jitter_factors, affine, mosaic_geom,
                                  mosaic_affine, fill3, mean3, std3, out, tmp, st);
}

// ---- Windowed resize in front of every chain above (k_window_h / k_window_h_list, k_window_v_norm / k_window_v_u8) ----
// workspace: that of the mosaic forms with max_rows in the place of Hin, [horizontal intermediate (B, max_rows, Wout, 3) | 8-bit image A |
// grey sums | 8-bit image B]: the windowed vertical pass writes the 8-bit window where the stage that follows expects the resized image.
size_t sd_preprocess_window_workspace_bytes(int B, int max_rows, int Hout, int Wout) {
    return sd_preprocess_mosaic_workspace_bytes(B, max_rows, 0, Hout, Wout);
}

static int window_check(const char* what, const uint8_t* images, int B, int Hin, int Win, int Hc, int Wc, int Hout, int Wout, const int* h_bounds,
                        const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const int* window, int max_rows, int max_cols,
                        const int* jitter_order, const float* jitter_factors, const double* affine, const int* mosaic_geom,
                        const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace,
                        size_t workspace_bytes) {
    if (int e = preprocess_check(what, images, B, Hin, Win, Hc, Wc, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, mean3, std3, out, workspace))
        return e;
    SD_REQUIRE(window, SD_ERR_INVALID, "%s: null window table", what);
    SD_REQUIRE(Hout > 0 && Wout > 0 && Hout <= Hc && Wout <= Wc, SD_ERR_INVALID, "%s: a %d x %d window does not fit a %d x %d canvas", what, Wout, Hout,
               Wc, Hc);
    SD_REQUIRE(max_rows > 0 && max_rows <= Hin && max_cols > 0 && max_cols <= Win, SD_ERR_INVALID,
               "%s: max_rows %d / max_cols %d should be in [1, %d] / [1, %d] (the source)", what, max_rows, max_cols, Hin, Win);
    SD_REQUIRE((jitter_order == nullptr) == (jitter_factors == nullptr), SD_ERR_INVALID,
               "%s: jitter_order and jitter_factors go together (both null = no jitter)", what);
    SD_REQUIRE((mosaic_geom == nullptr) == (mosaic_affine == nullptr), SD_ERR_INVALID,
               "%s: mosaic_geom and mosaic_affine go together (both null = no mosaic)", what);
    SD_REQUIRE(fill3 || !(affine || mosaic_geom), SD_ERR_INVALID, "%s: a warp or a mosaic needs a fill colour", what);
    SD_REQUIRE(B <= 65535 || !(jitter_order || affine || mosaic_geom), SD_ERR_INVALID, "%s: batch %d > 65535", what, B);
    SD_REQUIRE(workspace_bytes >= sd_preprocess_window_workspace_bytes(B, max_rows, Hout, Wout), SD_ERR_WORKSPACE, "%s: workspace %zu < %zu", what,
               workspace_bytes, sd_preprocess_window_workspace_bytes(B, max_rows, Hout, Wout));
    return 0;
}

// the launches after the horizontal pass: the windowed vertical pass, fused with Normalize when no stage follows, else into the 8-bit
// image the existing tails resample into, and then their launches (jitter_norm, affine_stages, mosaic_stages)
static int window_tail(int B, int Hc, int Wc, int Hout, int Wout, const int* v_bounds, const int* v_kk, int v_ksize, const int* window, int max_rows,
                       const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine, const int* mosaic_geom,
                       const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3, float* out, uint8_t* tmp,
                       hipStream_t st) {
    const dim3 grid(cdiv((int64_t)B * Hout * Wout, 256));
    if (!jitter_order && !affine && !mosaic_geom) {
        hipLaunchKernelGGL(k_window_v_norm, grid, dim3(256), 0, st, tmp, out, Hc, Wc, Hout, Wout, v_bounds, v_kk, v_ksize, window, max_rows, flips,
                           mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], B);
        SD_LAUNCH_CHECK();
        return 0;
    }
    uint8_t* img_a = tmp + sd_preprocess_workspace_bytes(B, max_rows, 0, Wout);
    unsigned long long* lsum = reinterpret_cast<unsigned long long*>(img_a + align_up((size_t)B * Hout * Wout * 3, 256));
    uint8_t* img_b = tmp + sd_preprocess_jitter_workspace_bytes(B, max_rows, 0, Hout, Wout);
    uint8_t* resized = (mosaic_geom != nullptr) == (affine != nullptr) ? img_a : img_b;    // jitter reads A, the warp B, the mosaic A with a warp, else B
    hipLaunchKernelGGL(k_window_v_u8, grid, dim3(256), 0, st, tmp, resized, Hc, Wc, Hout, Wout, v_bounds, v_kk, v_ksize, window, max_rows, B);
    SD_LAUNCH_CHECK();
    if (mosaic_geom)
        return mosaic_stages(B, Hout, Wout, flips, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, img_a,
                             img_b, lsum, st);
    if (affine)
        return affine_stages(B, Hout, Wout, flips, jitter_order, jitter_factors, affine, fill3, mean3, std3, out, resized, img_a, lsum, st);
    return jitter_norm(B, Hout, Wout, flips, jitter_order, jitter_factors, mean3, std3, out, img_a, lsum, st);
}

int sd_preprocess_images_window(const uint8_t* images, int B, int Hin, int Win, int Hc, int Wc, int Hout, int Wout, const int* h_bounds,
                                const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const int* window, int max_rows,
                                int max_cols, const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3,
                                float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    if (int e = window_check("sd_preprocess_images_window", images, B, Hin, Win, Hc, Wc, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                             window, max_rows, max_cols, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out,
                             workspace, workspace_bytes)) return e;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (jitter_order) {
        uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, max_rows, 0, Wout);
        SD_HIP(hipMemsetAsync(img + align_up((size_t)B * Hout * Wout * 3, 256), 0, (size_t)B * 8, st));    // lsum
    }
    hipLaunchKernelGGL(k_window_h, dim3(cdiv((int64_t)B * max_rows * Wout, 256)), dim3(256), 0, st, images, tmp, Hin, Win, Hc, Wc, Hout, Wout, h_bounds,
                       h_kk, h_ksize, v_bounds, window, max_rows, B);
    SD_LAUNCH_CHECK();
    return window_tail(B, Hc, Wc, Hout, Wout, v_bounds, v_kk, v_ksize, window, max_rows, flips, jitter_order, jitter_factors, affine, mosaic_geom,
                       mosaic_affine, fill3, mean3, std3, out, tmp, st);
}

int sd_preprocess_images_list_window(const uint8_t* const* images, int B, int Hin, int Win, int Hc, int Wc, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const int* window,
                                     int max_rows, int max_cols, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                     const double* affine, const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3,
                                     const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                     sd_stream_t stream) {
    const char* what = "sd_preprocess_images_list_window";
    if (int e = window_check(what, reinterpret_cast<const uint8_t*>(images), B, Hin, Win, Hc, Wc, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                             v_ksize, window, max_rows, max_cols, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3,
                             out, workspace, workspace_bytes)) return e;
    SD_REQUIRE((int64_t)max_cols * 3 + 32 <= HL_LDS_BYTES, SD_ERR_INVALID,
               "%s: a column span of %d source pixels exceeds the LDS staging buffer (at most %d)", what, max_cols, (HL_LDS_BYTES - 32) / 3);
    const int rpb = (int)std::min<int64_t>(HL_ROWS, (HL_LDS_BYTES - 32) / ((int64_t)max_cols * 3));
    const int bpi = cdiv(max_rows, rpb);
    SD_REQUIRE((int64_t)B * bpi < (1ll << 31), SD_ERR_INVALID, "%s: batch too large", what);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (jitter_order) {
        uint8_t* img = tmp + sd_preprocess_workspace_bytes(B, max_rows, 0, Wout);
        SD_HIP(hipMemsetAsync(img + align_up((size_t)B * Hout * Wout * 3, 256), 0, (size_t)B * 8, st));    // lsum
    }
    hipLaunchKernelGGL(k_window_h_list, dim3((unsigned)((int64_t)B * bpi)), dim3(256), (size_t)rpb * max_cols * 3 + 32, st, images, tmp, Win, Hc, Wc,
                       Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, window, max_rows, max_cols, rpb, bpi);
    SD_LAUNCH_CHECK();
    return window_tail(B, Hc, Wc, Hout, Wout, v_bounds, v_kk, v_ksize, window, max_rows, flips, jitter_order, jitter_factors, affine, mosaic_geom,
                       mosaic_affine, fill3, mean3, std3, out, tmp, st);
}

// ---- Letterbox in front of every chain above (k_resample_h / k_resample_h_list at Wout = Wi, k_letterbox_v_norm / k_letterbox_v_u8) ----
// workspace: [horizontal intermediate (B, Hin, Wi, 3) | 8-bit frame A | grey sums | 8-bit frame B], the layout of the mosaic forms with
// the intermediate at the inner width and the 8-bit images at the frame's size.
size_t sd_preprocess_letterbox_workspace_bytes(int B, int Hin, int Wi, int Hout, int Wout) {
    return align_up((size_t)B * Hin * Wi * 3, 256) + 2 * align_up((size_t)B * Hout * Wout * 3, 256) + align_up((size_t)B * 8, 256);
}

static int letterbox_check(const char* what, const uint8_t* images, int B, int Hin, int Win, int Hi, int Wi, int Hout, int Wout, int y0, int x0,
                           const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                           const int* jitter_order, const float* jitter_factors, const double* affine, const int* mosaic_geom,
                           const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace,
                           size_t workspace_bytes) {
    if (int e = preprocess_check(what, images, B, Hin, Win, Hi, Wi, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, mean3, std3, out, workspace))
        return e;
    SD_REQUIRE(fill3, SD_ERR_INVALID, "%s: null fill colour", what);
    SD_REQUIRE(Hout > 0 && Wout > 0 && (int64_t)B * Hout * Wout * 3 < (1ll << 40), SD_ERR_INVALID, "%s: bad frame %d x %d", what, Wout, Hout);
    SD_REQUIRE(x0 >= 0 && y0 >= 0 && (int64_t)x0 + Wi <= Wout && (int64_t)y0 + Hi <= Hout, SD_ERR_INVALID,
               "%s: a %d x %d image at (%d, %d) does not lie inside the %d x %d frame", what, Wi, Hi, x0, y0, Wout, Hout);
    SD_REQUIRE((jitter_order == nullptr) == (jitter_factors == nullptr), SD_ERR_INVALID,
               "%s: jitter_order and jitter_factors go together (both null = no jitter)", what);
    SD_REQUIRE((mosaic_geom == nullptr) == (mosaic_affine == nullptr), SD_ERR_INVALID,
               "%s: mosaic_geom and mosaic_affine go together (both null = no mosaic)", what);
    SD_REQUIRE(B <= 65535 || !(jitter_order || affine || mosaic_geom), SD_ERR_INVALID, "%s: batch %d > 65535", what, B);
    SD_REQUIRE(workspace_bytes >= sd_preprocess_letterbox_workspace_bytes(B, Hin, Wi, Hout, Wout), SD_ERR_WORKSPACE, "%s: workspace %zu < %zu", what,
               workspace_bytes, sd_preprocess_letterbox_workspace_bytes(B, Hin, Wi, Hout, Wout));
    return 0;
}

// the launches after the horizontal pass: the letterbox vertical pass, fused with Normalize when no stage follows, else into the 8-bit
// frame the existing tails resample into, and then their launches (jitter_norm, affine_stages, mosaic_stages) at the frame's size
static int letterbox_tail(int B, int Hin, int Hi, int Wi, int Hout, int Wout, int y0, int x0, const int* v_bounds, const int* v_kk, int v_ksize,
                          const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine, const int* mosaic_geom,
                          const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3, float* out, uint8_t* tmp,
                          hipStream_t st) {
    const dim3 grid(cdiv((int64_t)B * Hout * Wout, 256));
    const int f0 = fill3[0], f1 = fill3[1], f2 = fill3[2];
    if (!jitter_order && !affine && !mosaic_geom) {
        hipLaunchKernelGGL(k_letterbox_v_norm, grid, dim3(256), 0, st, tmp, out, Hin, Hi, Wi, Hout, Wout, y0, x0, v_bounds, v_kk, v_ksize, flips, f0,
                           f1, f2, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], B);
        SD_LAUNCH_CHECK();
        return 0;
    }
    const size_t frame = align_up((size_t)B * Hout * Wout * 3, 256);
    uint8_t* img_a = tmp + align_up((size_t)B * Hin * Wi * 3, 256);
    unsigned long long* lsum = reinterpret_cast<unsigned long long*>(img_a + frame);
    uint8_t* img_b = img_a + frame + align_up((size_t)B * 8, 256);
    uint8_t* framed = (mosaic_geom != nullptr) == (affine != nullptr) ? img_a : img_b;     // jitter reads A, the warp B, the mosaic A with a warp, else B
    hipLaunchKernelGGL(k_letterbox_v_u8, grid, dim3(256), 0, st, tmp, framed, Hin, Hi, Wi, Hout, Wout, y0, x0, v_bounds, v_kk, v_ksize, f0, f1, f2, B);
    SD_LAUNCH_CHECK();
    if (mosaic_geom)
        return mosaic_stages(B, Hout, Wout, flips, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, img_a,
                             img_b, lsum, st);
    if (affine)
        return affine_stages(B, Hout, Wout, flips, jitter_order, jitter_factors, affine, fill3, mean3, std3, out, framed, img_a, lsum, st);
    return jitter_norm(B, Hout, Wout, flips, jitter_order, jitter_factors, mean3, std3, out, img_a, lsum, st);
}

static int letterbox_zero_lsum(int B, int Hin, int Wi, int Hout, int Wout, uint8_t* tmp, hipStream_t st) {
    uint8_t* lsum = tmp + align_up((size_t)B * Hin * Wi * 3, 256) + align_up((size_t)B * Hout * Wout * 3, 256);
    SD_HIP(hipMemsetAsync(lsum, 0, (size_t)B * 8, st));
    return 0;
}

int sd_preprocess_images_letterbox(const uint8_t* images, int B, int Hin, int Win, int Hi, int Wi, int Hout, int Wout, int y0, int x0,
                                   const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                                   const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                   const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3,
                                   float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    if (int e = letterbox_check("sd_preprocess_images_letterbox", images, B, Hin, Win, Hi, Wi, Hout, Wout, y0, x0, h_bounds, h_kk, h_ksize, v_bounds,
                                v_kk, v_ksize, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace,
                                workspace_bytes)) return e;
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (jitter_order)
        if (int e = letterbox_zero_lsum(B, Hin, Wi, Hout, Wout, tmp, st)) return e;
    const int64_t rows = (int64_t)B * Hin;
    hipLaunchKernelGGL(k_resample_h, dim3(cdiv(rows * Wi, 256)), dim3(256), 0, st, images, tmp, Hin, Win, Wi, h_bounds, h_kk, h_ksize, rows);
    SD_LAUNCH_CHECK();
    return letterbox_tail(B, Hin, Hi, Wi, Hout, Wout, y0, x0, v_bounds, v_kk, v_ksize, flips, jitter_order, jitter_factors, affine, mosaic_geom,
                          mosaic_affine, fill3, mean3, std3, out, tmp, st);
}

int sd_preprocess_images_list_letterbox(const uint8_t* const* images, int B, int Hin, int Win, int Hi, int Wi, int Hout, int Wout, int y0, int x0,
                                        const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                                        const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                        const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3, const float* mean3,
                                        const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_list_letterbox";
    if (int e = letterbox_check(what, reinterpret_cast<const uint8_t*>(images), B, Hin, Win, Hi, Wi, Hout, Wout, y0, x0, h_bounds, h_kk, h_ksize,
                                v_bounds, v_kk, v_ksize, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out,
                                workspace, workspace_bytes)) return e;
    SD_REQUIRE((int64_t)Win * 3 + 32 <= HL_LDS_BYTES, SD_ERR_INVALID, "%s: source rows of %d pixels exceed the LDS staging buffer (at most %d)",
               what, Win, (HL_LDS_BYTES - 32) / 3);
    const int rpb = (int)std::min<int64_t>(HL_ROWS, (HL_LDS_BYTES - 32) / ((int64_t)Win * 3));
    const int bpi = cdiv(Hin, rpb);
    SD_REQUIRE((int64_t)B * bpi < (1ll << 31), SD_ERR_INVALID, "%s: batch too large", what);
    hipStream_t st = (hipStream_t)stream;
    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    if (jitter_order)
        if (int e = letterbox_zero_lsum(B, Hin, Wi, Hout, Wout, tmp, st)) return e;
    if (int e = resample_h_list(images, tmp, B, Hin, Win, Wi, h_bounds, h_kk, h_ksize, rpb, bpi, st)) return e;
    return letterbox_tail(B, Hin, Hi, Wi, Hout, Wout, y0, x0, v_bounds, v_kk, v_ksize, flips, jitter_order, jitter_factors, affine, mosaic_geom,
                          mosaic_affine, fill3, mean3, std3, out, tmp, st);
}

// ---- Gaussian blur between the warp and the jitter, behind any geometry (sd_blur.hip: blur_stage; k_u8_norm) ----
// workspace: [horizontal intermediate | 8-bit image A | grey sums | 8-bit image B] with the intermediate of the geometry, i.e. the layout of
// the mosaic, window and letterbox forms.  The 8-bit stages in front of the blur -- vertical pass [, mosaic] [, warp] -- alternate between
// A and B so that the last of them writes A: the blur's horizontal direction then writes B and its vertical direction A, where the jitter
// launches (and k_u8_norm) read.  No stage runs in place.
size_t sd_preprocess_blur_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0) {
    if (geometry == SD_GEOM_WINDOW) return sd_preprocess_window_workspace_bytes(B, g0, Hout, Wout);
    if (geometry == SD_GEOM_LETTERBOX) return sd_preprocess_letterbox_workspace_bytes(B, Hin, Wg, Hout, Wout);
    return sd_preprocess_mosaic_workspace_bytes(B, Hin, Win, Hout, Wout);
}

// the blur and perspective forms proper (blur or persp set): the checks of the geometry's entry point, its horizontal pass, its vertical
// pass into an 8-bit image, the 8-bit stages -- the warp slot is k_affine_u8 or k_persp_u8 --, the blur unless its table is null, the sensor
// noise unless its table is null (sd_noise.hip: noise_stage, on image A in place, no workspace), the JPEG
// round trip unless its table is null (sd_jpeg.hip: jpeg_stage, on image A in place; its planes lie behind image B), the tone stage unless
// its table is null (sd_tone.hip: tone_stage, on image A in place; its histograms and tables lie behind the planes), and the jitter or
// plain tail
static int preprocess_blur(const char* what, bool list, const void* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                           int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                           const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                           const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur, const int* jpeg,
                           const int* tone, const int* noise, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                           void* workspace, size_t workspace_bytes, hipStream_t st) {
    const double* warp = affine ? affine : persp;                        // one warp slot: the callers refuse both together
    const uint8_t* packed = reinterpret_cast<const uint8_t*>(images);
    const uint8_t* const* table = reinterpret_cast<const uint8_t* const*>(images);
    int rpb = 0, bpi = 0;
    size_t tmp_bytes = 0;
    if (geometry == SD_GEOM_STRETCH) {
        if (list) {
            if (int e = preprocess_list_check(what, table, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, mean3, std3, out,
                                              workspace, &rpb, &bpi)) return e;
        } else if (int e = preprocess_check(what, packed, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, mean3, std3, out,
                                            workspace)) return e;
        SD_REQUIRE(!window, SD_ERR_INVALID, "%s: a window table needs SD_GEOM_WINDOW", what);
        SD_REQUIRE((jitter_order == nullptr) == (jitter_factors == nullptr), SD_ERR_INVALID,
                   "%s: jitter_order and jitter_factors go together (both null = no jitter)", what);
        SD_REQUIRE((mosaic_geom == nullptr) == (mosaic_affine == nullptr), SD_ERR_INVALID,
                   "%s: mosaic_geom and mosaic_affine go together (both null = no mosaic)", what);
        SD_REQUIRE(fill3 || !(warp || mosaic_geom), SD_ERR_INVALID, "%s: a warp or a mosaic needs a fill colour", what);
        SD_REQUIRE(workspace_bytes >= sd_preprocess_mosaic_workspace_bytes(B, Hin, Win, Hout, Wout), SD_ERR_WORKSPACE, "%s: workspace %zu < %zu", what,
                   workspace_bytes, sd_preprocess_mosaic_workspace_bytes(B, Hin, Win, Hout, Wout));
        tmp_bytes = sd_preprocess_workspace_bytes(B, Hin, Win, Wout);
    } else if (geometry == SD_GEOM_WINDOW) {
        if (int e = window_check(what, packed, B, Hin, Win, Hg, Wg, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, window, g0, g1,
                                 jitter_order, jitter_factors, warp, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace, workspace_bytes))
            return e;
        if (list) {
            SD_REQUIRE((int64_t)g1 * 3 + 32 <= HL_LDS_BYTES, SD_ERR_INVALID,
                       "%s: a column span of %d source pixels exceeds the LDS staging buffer (at most %d)", what, g1, (HL_LDS_BYTES - 32) / 3);
            rpb = (int)std::min<int64_t>(HL_ROWS, (HL_LDS_BYTES - 32) / ((int64_t)g1 * 3));
            bpi = cdiv(g0, rpb);
            SD_REQUIRE((int64_t)B * bpi < (1ll << 31), SD_ERR_INVALID, "%s: batch too large", what);
        }
        tmp_bytes = sd_preprocess_workspace_bytes(B, g0, 0, Wout);
    } else if (geometry == SD_GEOM_LETTERBOX) {
        SD_REQUIRE(!window, SD_ERR_INVALID, "%s: a window table needs SD_GEOM_WINDOW", what);
        if (int e = letterbox_check(what, packed, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, jitter_order,
                                    jitter_factors, warp, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace, workspace_bytes)) return e;
        if (list) {
            SD_REQUIRE((int64_t)Win * 3 + 32 <= HL_LDS_BYTES, SD_ERR_INVALID, "%s: source rows of %d pixels exceed the LDS staging buffer (at most %d)",
                       what, Win, (HL_LDS_BYTES - 32) / 3);
            rpb = (int)std::min<int64_t>(HL_ROWS, (HL_LDS_BYTES - 32) / ((int64_t)Win * 3));
            bpi = cdiv(Hin, rpb);
            SD_REQUIRE((int64_t)B * bpi < (1ll << 31), SD_ERR_INVALID, "%s: batch too large", what);
        }
        tmp_bytes = align_up((size_t)B * Hin * Wg * 3, 256);
    } else {
        SD_REQUIRE(false, SD_ERR_INVALID, "%s: unknown geometry %d", what, geometry);
    }
    SD_REQUIRE(B <= 65535 && Hout <= 65535 * 64, SD_ERR_INVALID, "%s: batch %d > 65535 or frame too tall", what, B);
    const size_t planes_at = sd_preprocess_blur_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0);   // a multiple of 256
    if (jpeg) {
        SD_REQUIRE(Hout % 16 == 0 && Wout % 16 == 0, SD_ERR_INVALID, "%s: jpeg needs a frame of whole 16 x 16 MCUs, not %d x %d", what, Wout, Hout);
        SD_REQUIRE(aligned16(workspace), SD_ERR_INVALID, "%s: jpeg needs a 16-byte aligned workspace", what);
        SD_REQUIRE(workspace_bytes >= planes_at + jpeg_planes_bytes(B, Hout, Wout), SD_ERR_WORKSPACE, "%s: workspace %zu < %zu", what, workspace_bytes,
                   planes_at + jpeg_planes_bytes(B, Hout, Wout));
    }
    const size_t tone_at = planes_at + jpeg_planes_bytes(B, Hout, Wout);                                      // a multiple of 256
    if (tone) {
        SD_REQUIRE((int64_t)Hout * Wout < (1ll << 31), SD_ERR_INVALID, "%s: tone needs a frame of fewer than 2^31 pixels, not %d x %d", what, Wout, Hout);
        SD_REQUIRE(aligned16(workspace), SD_ERR_INVALID, "%s: tone needs a 16-byte aligned workspace", what);
        SD_REQUIRE(workspace_bytes >= tone_at + tone_workspace_bytes(B), SD_ERR_WORKSPACE, "%s: workspace %zu < %zu", what, workspace_bytes,
                   tone_at + tone_workspace_bytes(B));
    }

    if (noise)
        SD_REQUIRE((int64_t)Hout * Wout < (1ll << 31), SD_ERR_INVALID, "%s: noise needs a frame of fewer than 2^31 pixels, not %d x %d", what, Wout, Hout);

    uint8_t* tmp = reinterpret_cast<uint8_t*>(workspace);
    const size_t frame = align_up((size_t)B * Hout * Wout * 3, 256);
    uint8_t* img_a = tmp + tmp_bytes;
    unsigned long long* lsum = reinterpret_cast<unsigned long long*>(img_a + frame);
    uint8_t* img_b = img_a + frame + align_up((size_t)B * 8, 256);
    if (jitter_order) SD_HIP(hipMemsetAsync(lsum, 0, (size_t)B * 8, st));
    const int before = 1 + (mosaic_geom ? 1 : 0) + (warp ? 1 : 0);       // 8-bit images written in front of the blur; the last one is A
    int k = 0;
    auto next = [&]() { return ((before - 1 - k++) & 1) ? img_b : img_a; };
    uint8_t* cur = next();
    const dim3 flat(cdiv((int64_t)B * Hout * Wout, 256));
    const int f0 = fill3 ? fill3[0] : 0, f1 = fill3 ? fill3[1] : 0, f2 = fill3 ? fill3[2] : 0;
    if (geometry == SD_GEOM_STRETCH) {
        if (list) {
            if (int e = resample_h_list(table, tmp, B, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rpb, bpi, st)) return e;
        } else {
            const int64_t rows = (int64_t)B * Hin;
            hipLaunchKernelGGL(k_resample_h, dim3(cdiv(rows * Wout, 256)), dim3(256), 0, st, packed, tmp, Hin, Win, Wout, h_bounds, h_kk, h_ksize, rows);
            SD_LAUNCH_CHECK();
        }
        if (int e = resample_v_u8(B, Hin, Hout, Wout, v_bounds, v_kk, v_ksize, tmp, cur, st)) return e;
    } else if (geometry == SD_GEOM_WINDOW) {
        if (list)
            hipLaunchKernelGGL(k_window_h_list, dim3((unsigned)((int64_t)B * bpi)), dim3(256), (size_t)rpb * g1 * 3 + 32, st, table, tmp, Win, Hg, Wg, Hout,
                               Wout, h_bounds, h_kk, h_ksize, v_bounds, window, g0, g1, rpb, bpi);
        else
            hipLaunchKernelGGL(k_window_h, dim3(cdiv((int64_t)B * g0 * Wout, 256)), dim3(256), 0, st, packed, tmp, Hin, Win, Hg, Wg, Hout, Wout, h_bounds,
                               h_kk, h_ksize, v_bounds, window, g0, B);
        SD_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_window_v_u8, flat, dim3(256), 0, st, tmp, cur, Hg, Wg, Hout, Wout, v_bounds, v_kk, v_ksize, window, g0, B);
        SD_LAUNCH_CHECK();
    } else {
        if (list) {
            if (int e = resample_h_list(table, tmp, B, Hin, Win, Wg, h_bounds, h_kk, h_ksize, rpb, bpi, st)) return e;
        } else {
            const int64_t rows = (int64_t)B * Hin;
            hipLaunchKernelGGL(k_resample_h, dim3(cdiv(rows * Wg, 256)), dim3(256), 0, st, packed, tmp, Hin, Win, Wg, h_bounds, h_kk, h_ksize, rows);
            SD_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(k_letterbox_v_u8, flat, dim3(256), 0, st, tmp, cur, Hin, Hg, Wg, Hout, Wout, g0, g1, v_bounds, v_kk, v_ksize, f0, f1, f2, B);
        SD_LAUNCH_CHECK();
    }
    const dim3 grid(cdiv(Wout, AF_TX * AF_PX), cdiv(Hout, AF_TY), B);
    if (mosaic_geom) {
        uint8_t* dst = next();
        hipLaunchKernelGGL(k_mosaic_u8, grid, dim3(256), 0, st, cur, dst, Hout, Wout, mosaic_geom, mosaic_affine, f0, f1, f2);
        SD_LAUNCH_CHECK();
        cur = dst;
    }
    if (affine) {
        uint8_t* dst = next();
        hipLaunchKernelGGL(k_affine_u8, grid, dim3(256), 0, st, cur, dst, Hout, Wout, affine, f0, f1, f2);
        SD_LAUNCH_CHECK();
        cur = dst;
    }
    if (persp) {
        uint8_t* dst = next();
        hipLaunchKernelGGL(k_persp_u8, grid, dim3(256), 0, st, cur, dst, Hout, Wout, persp, f0, f1, f2);
        SD_LAUNCH_CHECK();
        cur = dst;
    }
    if (blur)                                                            // cur == img_a; without a blur the jitter reads it as it is
        if (int e = blur_stage(cur, img_b, img_a, B, Hout, Wout, blur, st)) return e;
    if (noise)                                                           // image A in place (with or without a blur the last stage wrote it)
        if (int e = noise_stage(img_a, img_a, B, Hout, Wout, noise, st)) return e;
    if (jpeg)                                                            // the last 8-bit image, in place: the second launch reads the planes only
        if (int e = jpeg_stage(img_a, img_a, tmp + planes_at, B, Hout, Wout, jpeg, st)) return e;
    if (tone)                                                            // in place as well: every byte is read and written by one thread
        if (int e = tone_stage(img_a, img_a, tmp + tone_at, B, Hout, Wout, tone, st)) return e;
    if (jitter_order) return jitter_norm(B, Hout, Wout, flips, jitter_order, jitter_factors, mean3, std3, out, img_a, lsum, st);
    hipLaunchKernelGGL(k_u8_norm, flat, dim3(256), 0, st, img_a, out, Hout, Wout, flips, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], B);
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_preprocess_images_blur(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const int* mosaic_geom, const double* mosaic_affine, const int* blur, const uint8_t* fill3,
                              const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_blur";
    if (blur)
        return preprocess_blur(what, false, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                               window, flips, jitter_order, jitter_factors, affine, nullptr, mosaic_geom, mosaic_affine, blur, nullptr, nullptr, nullptr, fill3, mean3, std3,
                               out, workspace, workspace_bytes, (hipStream_t)stream);
    if (geometry == SD_GEOM_WINDOW)
        return sd_preprocess_images_window(images, B, Hin, Win, Hg, Wg, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, window, g0, g1, flips,
                                           jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace,
                                           workspace_bytes, stream);
    if (geometry == SD_GEOM_LETTERBOX)
        return sd_preprocess_images_letterbox(images, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips,
                                              jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace,
                                              workspace_bytes, stream);
    SD_REQUIRE(geometry == SD_GEOM_STRETCH, SD_ERR_INVALID, "%s: unknown geometry %d", what, geometry);
    SD_REQUIRE((jitter_order == nullptr) == (jitter_factors == nullptr), SD_ERR_INVALID,
               "%s: jitter_order and jitter_factors go together (both null = no jitter)", what);
    if (mosaic_geom || mosaic_affine)
        return sd_preprocess_images_mosaic(images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips, jitter_order,
                                           jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace, workspace_bytes, stream);
    if (affine)
        return sd_preprocess_images_affine(images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips, jitter_order,
                                           jitter_factors, affine, fill3, mean3, std3, out, workspace, workspace_bytes, stream);
    if (jitter_order)
        return sd_preprocess_images_jitter(images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips, jitter_order,
                                           jitter_factors, mean3, std3, out, workspace, workspace_bytes, stream);
    return sd_preprocess_images(images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips, mean3, std3, out, workspace,
                                workspace_bytes, stream);
}

int sd_preprocess_images_list_blur(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const int* mosaic_geom, const double* mosaic_affine, const int* blur, const uint8_t* fill3,
                                   const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_list_blur";
    if (blur)
        return preprocess_blur(what, true, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                               window, flips, jitter_order, jitter_factors, affine, nullptr, mosaic_geom, mosaic_affine, blur, nullptr, nullptr, nullptr, fill3, mean3, std3,
                               out, workspace, workspace_bytes, (hipStream_t)stream);
    if (geometry == SD_GEOM_WINDOW)
        return sd_preprocess_images_list_window(images, B, Hin, Win, Hg, Wg, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, window, g0, g1,
                                                flips, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace,
                                                workspace_bytes, stream);
    if (geometry == SD_GEOM_LETTERBOX)
        return sd_preprocess_images_list_letterbox(images, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips,
                                                   jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace,
                                                   workspace_bytes, stream);
    SD_REQUIRE(geometry == SD_GEOM_STRETCH, SD_ERR_INVALID, "%s: unknown geometry %d", what, geometry);
    SD_REQUIRE((jitter_order == nullptr) == (jitter_factors == nullptr), SD_ERR_INVALID,
               "%s: jitter_order and jitter_factors go together (both null = no jitter)", what);
    if (mosaic_geom || mosaic_affine)
        return sd_preprocess_images_list_mosaic(images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips, jitter_order,
                                                jitter_factors, affine, mosaic_geom, mosaic_affine, fill3, mean3, std3, out, workspace, workspace_bytes,
                                                stream);
    if (affine)
        return sd_preprocess_images_list_affine(images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips, jitter_order,
                                                jitter_factors, affine, fill3, mean3, std3, out, workspace, workspace_bytes, stream);
    if (jitter_order)
        return sd_preprocess_images_list_jitter(images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips, jitter_order,
                                                jitter_factors, mean3, std3, out, workspace, workspace_bytes, stream);
    return sd_preprocess_images_list(images, B, Hin, Win, Hout, Wout, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize, flips, mean3, std3, out, workspace,
                                     workspace_bytes, stream);
}

// ---- RandomPerspective in the warp slot of the chain (k_persp_u8), behind any geometry ----
// persp null: the blur form, a call.  persp set: the host has folded the affine draw into the homography, so affine must be null; the
// chain is preprocess_blur's with k_persp_u8 as the warp and the blur optional.
int sd_perspective_u8(const uint8_t* in, uint8_t* out, int B, int H, int W, const double* coeffs, const uint8_t* fill3, sd_stream_t stream) {
    SD_REQUIRE(in && out && coeffs && fill3, SD_ERR_INVALID, "sd_perspective_u8: null pointer");
    SD_REQUIRE(B > 0 && H > 0 && W > 0, SD_ERR_INVALID, "sd_perspective_u8: bad shape");
    SD_REQUIRE(B <= 65535 && H <= 65535 * AF_TY && (int64_t)B * H * W * 3 < (1ll << 40), SD_ERR_INVALID, "sd_perspective_u8: batch too large");
    const int64_t bytes = (int64_t)B * H * W * 3;
    SD_REQUIRE(in + bytes <= out || out + bytes <= in, SD_ERR_INVALID, "sd_perspective_u8: in place is not supported (out must not overlap in)");
    const dim3 grid(cdiv(W, AF_TX * AF_PX), cdiv(H, AF_TY), B);
    hipLaunchKernelGGL(k_persp_u8, grid, dim3(256), 0, (hipStream_t)stream, in, out, H, W, coeffs, (int)fill3[0], (int)fill3[1], (int)fill3[2]);
    SD_LAUNCH_CHECK();
    return 0;
}

int sd_preprocess_images_persp(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                               const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                               const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                               const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                               const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                               sd_stream_t stream) {
    const char* what = "sd_preprocess_images_persp";
    if (!persp)
        return sd_preprocess_images_blur(images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                                         window, flips, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, blur, fill3, mean3, std3, out,
                                         workspace, workspace_bytes, stream);
    SD_REQUIRE(!affine, SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    SD_REQUIRE(fill3, SD_ERR_INVALID, "%s: a warp needs a fill colour", what);
    return preprocess_blur(what, false, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                           window, flips, jitter_order, jitter_factors, nullptr, persp, mosaic_geom, mosaic_affine, blur, nullptr, nullptr, nullptr, fill3, mean3, std3, out,
                           workspace, workspace_bytes, (hipStream_t)stream);
}

int sd_preprocess_images_list_persp(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                    int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                    int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                    const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                    const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace,
                                    size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_list_persp";
    if (!persp)
        return sd_preprocess_images_list_blur(images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                              v_ksize, window, flips, jitter_order, jitter_factors, affine, mosaic_geom, mosaic_affine, blur, fill3,
                                              mean3, std3, out, workspace, workspace_bytes, stream);
    SD_REQUIRE(!affine, SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    SD_REQUIRE(fill3, SD_ERR_INVALID, "%s: a warp needs a fill colour", what);
    return preprocess_blur(what, true, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                           window, flips, jitter_order, jitter_factors, nullptr, persp, mosaic_geom, mosaic_affine, blur, nullptr, nullptr, nullptr, fill3, mean3, std3, out,
                           workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- JPEG round trip between the blur and the jitter (sd_jpeg.hip: jpeg_stage), behind any geometry ----
// jpeg null: the perspective form, a call.  jpeg set: preprocess_blur's chain with the one more stage, every other table optional;
// workspace: the blur form's, then the decoded planes.
size_t sd_preprocess_jpeg_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0) {
    if (B <= 0 || Hout <= 0 || Wout <= 0) return sd_preprocess_blur_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0);
    return sd_preprocess_blur_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0) + jpeg_planes_bytes(B, Hout, Wout);
}

int sd_preprocess_images_jpeg(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                              const int* jpeg, const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace,
                              size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_jpeg";
    if (!jpeg)
        return sd_preprocess_images_persp(images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                                          window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, fill3, mean3,
                                          std3, out, workspace, workspace_bytes, stream);
    SD_REQUIRE(!(affine && persp), SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    return preprocess_blur(what, false, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                           window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, jpeg, nullptr, nullptr, fill3, mean3, std3, out,
                           workspace, workspace_bytes, (hipStream_t)stream);
}

int sd_preprocess_images_list_jpeg(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                   const int* jpeg, const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace,
                                   size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_list_jpeg";
    if (!jpeg)
        return sd_preprocess_images_list_persp(images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                               v_ksize, window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur,
                                               fill3, mean3, std3, out, workspace, workspace_bytes, stream);
    SD_REQUIRE(!(affine && persp), SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    return preprocess_blur(what, true, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                           window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, jpeg, nullptr, nullptr, fill3, mean3, std3, out,
                           workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- histogram tone curves between the JPEG round trip and the jitter (sd_tone.hip: tone_stage), behind any geometry ----
// tone null: the JPEG form, a call.  tone set: preprocess_blur's chain with the one more stage, every other table optional;
// workspace: the JPEG form's, then the histograms and the tables.
size_t sd_preprocess_tone_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0) {
    if (B <= 0 || Hout <= 0 || Wout <= 0) return sd_preprocess_jpeg_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0);
    return sd_preprocess_jpeg_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0) + tone_workspace_bytes(B);
}

int sd_preprocess_images_tone(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                              const int* jpeg, const int* tone, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                              void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_tone";
    if (!tone)
        return sd_preprocess_images_jpeg(images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                                         window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, jpeg, fill3,
                                         mean3, std3, out, workspace, workspace_bytes, stream);
    SD_REQUIRE(!(affine && persp), SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    return preprocess_blur(what, false, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                           window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, jpeg, tone, nullptr, fill3, mean3, std3,
                           out, workspace, workspace_bytes, (hipStream_t)stream);
}

int sd_preprocess_images_list_tone(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                   const int* jpeg, const int* tone, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                                   void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_list_tone";
    if (!tone)
        return sd_preprocess_images_list_jpeg(images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                              v_ksize, window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur,
                                              jpeg, fill3, mean3, std3, out, workspace, workspace_bytes, stream);
    SD_REQUIRE(!(affine && persp), SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    return preprocess_blur(what, true, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                           window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, jpeg, tone, nullptr, fill3, mean3, std3,
                           out, workspace, workspace_bytes, (hipStream_t)stream);
}

// ---- sensor noise between the blur and the JPEG round trip (sd_noise.hip: noise_stage), behind any geometry ----
// noise null: the tone form, a call.  noise set: preprocess_blur's chain with the one more stage, every other table optional;
// workspace: the tone form's (the stage needs none).
size_t sd_preprocess_noise_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0) {
    return sd_preprocess_tone_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0);
}

int sd_preprocess_images_noise(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                               const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                               const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                               const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                               const int* jpeg, const int* tone, const int* noise, const uint8_t* fill3, const float* mean3, const float* std3,
                               float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_noise";
    if (!noise)
        return sd_preprocess_images_tone(images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                                         window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, jpeg, tone,
                                         fill3, mean3, std3, out, workspace, workspace_bytes, stream);
    SD_REQUIRE(!(affine && persp), SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    return preprocess_blur(what, false, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                           window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, jpeg, tone, noise, fill3, mean3,
                           std3, out, workspace, workspace_bytes, (hipStream_t)stream);
}

int sd_preprocess_images_list_noise(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                    int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                    int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                    const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                    const int* jpeg, const int* tone, const int* noise, const uint8_t* fill3, const float* mean3, const float* std3,
                                    float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    const char* what = "sd_preprocess_images_list_noise";
    if (!noise)
        return sd_preprocess_images_list_tone(images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk,
                                              v_ksize, window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur,
                                              jpeg, tone, fill3, mean3, std3, out, workspace, workspace_bytes, stream);
    SD_REQUIRE(!(affine && persp), SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    return preprocess_blur(what, true, images, geometry, B, Hin, Win, Hg, Wg, Hout, Wout, g0, g1, h_bounds, h_kk, h_ksize, v_bounds, v_kk, v_ksize,
                           window, flips, jitter_order, jitter_factors, affine, persp, mosaic_geom, mosaic_affine, blur, jpeg, tone, noise, fill3, mean3,
                           std3, out, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
