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

// ---- the legacy size queries: the chain's workspace layout (below) with the regions their forms use --------------------------------
size_t sd_preprocess_workspace_bytes(int B, int Hin, int Win, int Wout) { return align_up((size_t)B * Hin * Wout * 3, 256); }

size_t sd_preprocess_jitter_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout) {
    return sd_preprocess_workspace_bytes(B, Hin, Win, Wout) + align_up((size_t)B * Hout * Wout * 3, 256) + align_up((size_t)B * 8, 256);
}

size_t sd_preprocess_affine_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout) {
    return sd_preprocess_jitter_workspace_bytes(B, Hin, Win, Hout, Wout) + align_up((size_t)B * Hout * Wout * 3, 256);
}

size_t sd_preprocess_mosaic_workspace_bytes(int B, int Hin, int Win, int Hout, int Wout) {
    return sd_preprocess_affine_workspace_bytes(B, Hin, Win, Hout, Wout);
}

size_t sd_preprocess_window_workspace_bytes(int B, int max_rows, int Hout, int Wout) {
    return sd_preprocess_mosaic_workspace_bytes(B, max_rows, 0, Hout, Wout);
}

size_t sd_preprocess_letterbox_workspace_bytes(int B, int Hin, int Wi, int Hout, int Wout) {
    return align_up((size_t)B * Hin * Wi * 3, 256) + 2 * align_up((size_t)B * Hout * Wout * 3, 256) + align_up((size_t)B * 8, 256);
}

size_t sd_preprocess_blur_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0) {
    if (geometry == SD_GEOM_WINDOW) return sd_preprocess_window_workspace_bytes(B, g0, Hout, Wout);
    if (geometry == SD_GEOM_LETTERBOX) return sd_preprocess_letterbox_workspace_bytes(B, Hin, Wg, Hout, Wout);
    return sd_preprocess_mosaic_workspace_bytes(B, Hin, Win, Hout, Wout);
}

size_t sd_preprocess_jpeg_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0) {
    if (B <= 0 || Hout <= 0 || Wout <= 0) return sd_preprocess_blur_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0);
    return sd_preprocess_blur_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0) + jpeg_planes_bytes(B, Hout, Wout);
}

size_t sd_preprocess_tone_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0) {
    if (B <= 0 || Hout <= 0 || Wout <= 0) return sd_preprocess_jpeg_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0);
    return sd_preprocess_jpeg_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0) + tone_workspace_bytes(B);
}

size_t sd_preprocess_noise_workspace_bytes(int geometry, int B, int Hin, int Win, int Wg, int Hout, int Wout, int g0) {
    return sd_preprocess_tone_workspace_bytes(geometry, B, Hin, Win, Wg, Hout, Wout, g0);
}

// ---- the preprocess chain: one descriptor (sd_preprocess_desc), one plan, one launcher ----------------------------------------------
//     H (horizontal resize) -> V (vertical resize [+ window | letterbox paste]) -> [mosaic] -> [affine | persp] -> [blur] -> [noise]
//     -> [jpeg] -> [tone] -> [jitter] -> flips -> Normalize
// plan_chain is host arithmetic only: the checks, the list form's LDS staging, the workspace layout and the launches with their buffers.
// sd_preprocess_chain and every legacy entry point run it under their own name and walk it (launch_chain); sd_preprocess_kernel_names
// prints it; sd_preprocess_chain_workspace_bytes is its ws_bytes.
//
// workspace: [horizontal intermediate (tmp) | 8-bit image A | grey sums | 8-bit image B | JPEG planes | tone histograms], every region a
// multiple of 256 bytes.  The plain stretch needs tmp only and the stretch with jitter alone up to the grey sums; every other plan
// reserves up to B's end (the window and letterbox forms always did), the planes with jpeg, the histograms -- behind the planes' place,
// set or not -- with tone.
//
// The A/B rule: the 8-bit stages in front of the blur -- V [, mosaic] [, warp] -- alternate between A and B so that the last of them
// writes A, where the blur (A -> B -> A), the in-place stages, the jitter and k_u8_norm read.  Without a late stage (persp, blur, noise,
// jpeg, tone) and without jitter that last stage is its kernel fused with flips + Normalize (`_norm`) and writes `out` instead.
enum ChainOp { OP_MEMSET, OP_H, OP_V, OP_MOSAIC, OP_AFFINE, OP_PERSP, OP_BLUR, OP_NOISE, OP_JPEG, OP_TONE, OP_LSUM, OP_JITTER_NORM, OP_U8_NORM };
enum ChainBuf { BUF_TMP, BUF_A, BUF_B, BUF_OUT, BUF_SUMS };
struct ChainStep { ChainOp op; ChainBuf src, dst; };                     // dst == BUF_OUT on V / MOSAIC / AFFINE: the `_norm` kernel, else `_u8`
struct ChainPlan {
    ChainStep steps[12];
    int n;
    int rows, cols;              // the horizontal intermediate is (B, rows, cols, 3)
    int span, rpb, bpi;          // list form: source pixels staged per row, source rows per block, blocks per image
    size_t a_at, sums_at, b_at, planes_at, tone_at, ws_bytes;
};
struct ChainDims { dim3 grid; size_t lds; };                             // every block has 256 threads; lds: dynamic bytes

static int plan_chain(const sd_preprocess_desc* desc, const char* what, ChainPlan* p) {
    SD_REQUIRE(desc, SD_ERR_INVALID, "%s: null descriptor", what);
    const sd_preprocess_desc& d = *desc;
    SD_REQUIRE(d.images && d.out && d.h_bounds && d.h_kk && d.v_bounds && d.v_kk && d.mean3 && d.std3, SD_ERR_INVALID, "%s: null pointer", what);
    SD_REQUIRE(d.geometry == SD_GEOM_STRETCH || d.geometry == SD_GEOM_WINDOW || d.geometry == SD_GEOM_LETTERBOX, SD_ERR_INVALID,
               "%s: unknown geometry %d", what, d.geometry);
    const bool window = d.geometry == SD_GEOM_WINDOW, letterbox = d.geometry == SD_GEOM_LETTERBOX;
    const int B = d.B, Hin = d.Hin, Win = d.Win, Hout = d.Hout, Wout = d.Wout;
    const int Ht = window || letterbox ? d.Hg : Hout, Wt = window || letterbox ? d.Wg : Wout;    // the resize target of the tables
    SD_REQUIRE(B > 0 && Hin > 0 && Win > 0 && Ht > 0 && Wt > 0 && d.h_ksize > 0 && d.v_ksize > 0, SD_ERR_INVALID, "%s: bad shape", what);
    SD_REQUIRE((int64_t)B * std::max(Hin, Ht) * std::max(Win, Wt) * 3 < (1ll << 40), SD_ERR_INVALID, "%s: batch too large", what);
    SD_REQUIRE(d.std3[0] != 0.f && d.std3[1] != 0.f && d.std3[2] != 0.f, SD_ERR_INVALID, "%s: zero std", what);
    SD_REQUIRE(window || !d.window, SD_ERR_INVALID, "%s: a window table needs SD_GEOM_WINDOW", what);
    if (window) {                                                        // (Hg, Wg) = the canvas, g0 / g1 = max_rows / max_cols
        SD_REQUIRE(d.window, SD_ERR_INVALID, "%s: null window table", what);
        SD_REQUIRE(Hout > 0 && Wout > 0 && Hout <= d.Hg && Wout <= d.Wg, SD_ERR_INVALID, "%s: a %d x %d window does not fit a %d x %d canvas", what,
                   Wout, Hout, d.Wg, d.Hg);
        SD_REQUIRE(d.g0 > 0 && d.g0 <= Hin && d.g1 > 0 && d.g1 <= Win, SD_ERR_INVALID,
                   "%s: max_rows %d / max_cols %d should be in [1, %d] / [1, %d] (the source)", what, d.g0, d.g1, Hin, Win);
    }
    if (letterbox) {                                                     // (Hg, Wg) = the inner image, g0 / g1 = y0 / x0
        SD_REQUIRE(d.fill3, SD_ERR_INVALID, "%s: null fill colour", what);
        SD_REQUIRE(Hout > 0 && Wout > 0 && (int64_t)B * Hout * Wout * 3 < (1ll << 40), SD_ERR_INVALID, "%s: bad frame %d x %d", what, Wout, Hout);
        SD_REQUIRE(d.g1 >= 0 && d.g0 >= 0 && (int64_t)d.g1 + d.Wg <= Wout && (int64_t)d.g0 + d.Hg <= Hout, SD_ERR_INVALID,
                   "%s: a %d x %d image at (%d, %d) does not lie inside the %d x %d frame", what, d.Wg, d.Hg, d.g1, d.g0, Wout, Hout);
    }
    SD_REQUIRE(!(d.affine && d.persp), SD_ERR_INVALID, "%s: persp and affine do not combine (fold the affine matrix into the homography)", what);
    SD_REQUIRE((d.jitter_order == nullptr) == (d.jitter_factors == nullptr), SD_ERR_INVALID,
               "%s: jitter_order and jitter_factors go together (both null = no jitter)", what);
    SD_REQUIRE((d.mosaic_geom == nullptr) == (d.mosaic_affine == nullptr), SD_ERR_INVALID,
               "%s: mosaic_geom and mosaic_affine go together (both null = no mosaic)", what);
    const bool jitter = d.jitter_order, mosaic = d.mosaic_geom, warp = d.affine || d.persp;
    const bool late = d.persp || d.blur || d.noise || d.jpeg || d.tone;
    SD_REQUIRE(d.fill3 || !(warp || mosaic), SD_ERR_INVALID, "%s: a warp or a mosaic needs a fill colour", what);
    // B is a grid dimension of the jitter, warp, mosaic and late launches (the late ones also take cdiv(Hout, 64)); the resize has flat grids
    SD_REQUIRE(B <= 65535 || !(jitter || warp || mosaic || late), SD_ERR_INVALID, "%s: batch %d > 65535", what, B);
    SD_REQUIRE(Hout <= 65535 * 64 || !late, SD_ERR_INVALID, "%s: a frame of %d rows is too tall", what, Hout);
    SD_REQUIRE((int64_t)Hout * Wout < (1ll << 31) || !(d.noise || d.tone), SD_ERR_INVALID,
               "%s: noise and tone need a frame of fewer than 2^31 pixels, not %d x %d", what, Wout, Hout);
    SD_REQUIRE(!d.jpeg || (Hout % 16 == 0 && Wout % 16 == 0), SD_ERR_INVALID, "%s: jpeg needs a frame of whole 16 x 16 MCUs, not %d x %d", what, Wout,
               Hout);

    p->rows = window ? d.g0 : Hin;
    p->cols = letterbox ? d.Wg : Wout;
    p->span = window ? d.g1 : Win;
    p->rpb = p->bpi = 0;
    if (d.list) {                                                        // a block stages rpb rows of span source pixels in LDS
        SD_REQUIRE((int64_t)p->span * 3 + 32 <= HL_LDS_BYTES, SD_ERR_INVALID,
                   "%s: source rows (or a window's column span) of %d pixels exceed the LDS staging buffer (at most %d)", what, p->span,
                   (HL_LDS_BYTES - 32) / 3);
        p->rpb = (int)std::min<int64_t>(HL_ROWS, (HL_LDS_BYTES - 32) / ((int64_t)p->span * 3));
        p->bpi = cdiv(p->rows, p->rpb);
        SD_REQUIRE((int64_t)B * p->bpi < (1ll << 31), SD_ERR_INVALID, "%s: batch too large", what);
    }

    const int stages = 1 + (mosaic ? 1 : 0) + (warp ? 1 : 0);            // 8-bit images written in front of the blur
    const bool fuse = !late && !jitter;
    const size_t frame = align_up((size_t)B * Hout * Wout * 3, 256);
    p->a_at = align_up((size_t)B * p->rows * p->cols * 3, 256);
    p->sums_at = p->a_at + frame;
    p->b_at = p->sums_at + align_up((size_t)B * 8, 256);
    p->planes_at = p->b_at + frame;
    p->tone_at = p->planes_at + jpeg_planes_bytes(B, Hout, Wout);
    const bool tmp_only = d.geometry == SD_GEOM_STRETCH && fuse && stages == 1, to_sums = d.geometry == SD_GEOM_STRETCH && !late && stages == 1;
    p->ws_bytes = d.tone ? p->tone_at + tone_workspace_bytes(B) : d.jpeg ? p->tone_at : tmp_only ? p->a_at : to_sums ? p->b_at : p->planes_at;

    p->n = 0;
    auto add = [&](ChainOp op, ChainBuf src, ChainBuf dst) { p->steps[p->n++] = ChainStep{op, src, dst}; };
    if (jitter) add(OP_MEMSET, BUF_SUMS, BUF_SUMS);
    add(OP_H, BUF_TMP, BUF_TMP);
    const ChainOp stage[3] = {OP_V, OP_MOSAIC, d.affine ? OP_AFFINE : OP_PERSP};
    const bool on[3] = {true, mosaic, warp};
    ChainBuf cur = BUF_TMP;
    for (int i = 0, left = stages; i < 3; ++i) {
        if (!on[i]) continue;
        --left;                                                          // stages still to come: an even number ends in A from A
        const ChainBuf dst = fuse && left == 0 ? BUF_OUT : (left & 1) ? BUF_B : BUF_A;
        add(stage[i], cur, dst);
        cur = dst;
    }
    if (d.blur) add(OP_BLUR, BUF_A, BUF_A);                              // through B
    if (d.noise) add(OP_NOISE, BUF_A, BUF_A);
    if (d.jpeg) add(OP_JPEG, BUF_A, BUF_A);
    if (d.tone) add(OP_TONE, BUF_A, BUF_A);
    if (jitter) {
        add(OP_LSUM, BUF_A, BUF_SUMS);
        add(OP_JITTER_NORM, BUF_A, BUF_OUT);
    } else if (late) {
        add(OP_U8_NORM, BUF_A, BUF_OUT);
    }
    return 0;
}

static ChainDims chain_dims(const sd_preprocess_desc& d, const ChainPlan& p, ChainOp op) {
    const int64_t npix = (int64_t)d.Hout * d.Wout;
    switch (op) {
    case OP_H:
        if (d.list) return {dim3((unsigned)((int64_t)d.B * p.bpi)), (size_t)p.rpb * p.span * 3 + 32};
        return {dim3(cdiv((int64_t)d.B * p.rows * p.cols, 256)), 0};
    case OP_MOSAIC: case OP_AFFINE: case OP_PERSP: return {dim3(cdiv(d.Wout, AF_TX * AF_PX), cdiv(d.Hout, AF_TY), d.B), 0};
    case OP_LSUM: return {dim3(std::min<int64_t>(cdiv(npix, 256), 64), d.B), 0};
    default: return {dim3(cdiv((int64_t)d.B * npix, 256)), 0};
    }
}

// the name of a step's kernel, or of a late stage (its launches belong to its own file), or "memset"
static const char* chain_name(const sd_preprocess_desc& d, const ChainStep& s) {
    const bool window = d.geometry == SD_GEOM_WINDOW, fused = s.dst == BUF_OUT;
    switch (s.op) {
    case OP_MEMSET: return "memset";
    case OP_H: return window ? (d.list ? "k_window_h_list" : "k_window_h") : (d.list ? "k_resample_h_list" : "k_resample_h");
    case OP_V:
        if (window) return fused ? "k_window_v_norm" : "k_window_v_u8";
        if (d.geometry == SD_GEOM_LETTERBOX) return fused ? "k_letterbox_v_norm" : "k_letterbox_v_u8";
        return fused ? "k_resample_v_norm" : "k_resample_v_u8";
    case OP_MOSAIC: return fused ? "k_mosaic_norm" : "k_mosaic_u8";
    case OP_AFFINE: return fused ? "k_affine_norm" : "k_affine_u8";
    case OP_PERSP: return "k_persp_u8";
    case OP_BLUR: return "blur";
    case OP_NOISE: return "noise";
    case OP_JPEG: return "jpeg";
    case OP_TONE: return "tone";
    case OP_LSUM: return "k_jitter_lsum";
    case OP_JITTER_NORM: return "k_jitter_norm";
    case OP_U8_NORM: return "k_u8_norm";
    }
    return "?";
}

static int launch_chain(const sd_preprocess_desc& d, const ChainPlan& p, uint8_t* ws, hipStream_t st) {
    uint8_t* const buf[] = {ws, ws + p.a_at, ws + p.b_at, nullptr, ws + p.sums_at};
    unsigned long long* sums = reinterpret_cast<unsigned long long*>(ws + p.sums_at);
    const uint8_t* packed = reinterpret_cast<const uint8_t*>(d.images);
    const uint8_t* const* table = reinterpret_cast<const uint8_t* const*>(d.images);
    const int B = d.B, Hin = d.Hin, Win = d.Win, Hg = d.Hg, Wg = d.Wg, Hout = d.Hout, Wout = d.Wout, g0 = d.g0, g1 = d.g1;
    const int f0 = d.fill3 ? d.fill3[0] : 0, f1 = d.fill3 ? d.fill3[1] : 0, f2 = d.fill3 ? d.fill3[2] : 0;
    const float m0 = d.mean3[0], m1 = d.mean3[1], m2 = d.mean3[2], s0 = d.std3[0], s1 = d.std3[1], s2 = d.std3[2];
    const dim3 block(256);
    for (int i = 0; i < p.n; ++i) {
        const ChainStep& s = p.steps[i];
        const ChainDims l = chain_dims(d, p, s.op);
        const uint8_t* src = buf[s.src];
        uint8_t* dst = buf[s.dst];
        const bool fused = s.dst == BUF_OUT;
        switch (s.op) {
        case OP_MEMSET: SD_HIP(hipMemsetAsync(sums, 0, (size_t)B * 8, st)); continue;
        case OP_H:
            if (d.geometry == SD_GEOM_WINDOW) {
                if (d.list)
                    hipLaunchKernelGGL(k_window_h_list, l.grid, block, l.lds, st, table, dst, Win, Hg, Wg, Hout, Wout, d.h_bounds, d.h_kk, d.h_ksize,
                                       d.v_bounds, d.window, g0, g1, p.rpb, p.bpi);
                else
                    hipLaunchKernelGGL(k_window_h, l.grid, block, 0, st, packed, dst, Hin, Win, Hg, Wg, Hout, Wout, d.h_bounds, d.h_kk, d.h_ksize,
                                       d.v_bounds, d.window, g0, B);
            } else if (d.list) {
                hipLaunchKernelGGL(k_resample_h_list, l.grid, block, l.lds, st, table, dst, Hin, Win, p.cols, d.h_bounds, d.h_kk, d.h_ksize, p.rpb, p.bpi);
            } else {
                hipLaunchKernelGGL(k_resample_h, l.grid, block, 0, st, packed, dst, Hin, Win, p.cols, d.h_bounds, d.h_kk, d.h_ksize, (int64_t)B * Hin);
            }
            break;
        case OP_V:
            if (d.geometry == SD_GEOM_WINDOW) {
                if (fused)
                    hipLaunchKernelGGL(k_window_v_norm, l.grid, block, 0, st, src, d.out, Hg, Wg, Hout, Wout, d.v_bounds, d.v_kk, d.v_ksize, d.window, g0,
                                       d.flips, m0, m1, m2, s0, s1, s2, B);
                else
                    hipLaunchKernelGGL(k_window_v_u8, l.grid, block, 0, st, src, dst, Hg, Wg, Hout, Wout, d.v_bounds, d.v_kk, d.v_ksize, d.window, g0, B);
            } else if (d.geometry == SD_GEOM_LETTERBOX) {
                if (fused)
                    hipLaunchKernelGGL(k_letterbox_v_norm, l.grid, block, 0, st, src, d.out, Hin, Hg, Wg, Hout, Wout, g0, g1, d.v_bounds, d.v_kk,
                                       d.v_ksize, d.flips, f0, f1, f2, m0, m1, m2, s0, s1, s2, B);
                else
                    hipLaunchKernelGGL(k_letterbox_v_u8, l.grid, block, 0, st, src, dst, Hin, Hg, Wg, Hout, Wout, g0, g1, d.v_bounds, d.v_kk, d.v_ksize,
                                       f0, f1, f2, B);
            } else if (fused) {
                hipLaunchKernelGGL(k_resample_v_norm, l.grid, block, 0, st, src, d.out, Hin, Hout, Wout, d.v_bounds, d.v_kk, d.v_ksize, d.flips, m0, m1,
                                   m2, s0, s1, s2, B);
            } else {
                hipLaunchKernelGGL(k_resample_v_u8, l.grid, block, 0, st, src, dst, Hin, Hout, Wout, d.v_bounds, d.v_kk, d.v_ksize, B);
            }
            break;
        case OP_MOSAIC:
            if (fused)
                hipLaunchKernelGGL(k_mosaic_norm, l.grid, block, 0, st, src, d.out, Hout, Wout, d.mosaic_geom, d.mosaic_affine, f0, f1, f2, d.flips, m0,
                                   m1, m2, s0, s1, s2);
            else
                hipLaunchKernelGGL(k_mosaic_u8, l.grid, block, 0, st, src, dst, Hout, Wout, d.mosaic_geom, d.mosaic_affine, f0, f1, f2);
            break;
        case OP_AFFINE:
            if (fused)
                hipLaunchKernelGGL(k_affine_norm, l.grid, block, 0, st, src, d.out, Hout, Wout, d.affine, f0, f1, f2, d.flips, m0, m1, m2, s0, s1, s2);
            else
                hipLaunchKernelGGL(k_affine_u8, l.grid, block, 0, st, src, dst, Hout, Wout, d.affine, f0, f1, f2);
            break;
        case OP_PERSP: hipLaunchKernelGGL(k_persp_u8, l.grid, block, 0, st, src, dst, Hout, Wout, d.persp, f0, f1, f2); break;
        case OP_BLUR: if (int e = blur_stage(src, buf[BUF_B], dst, B, Hout, Wout, d.blur, st)) return e; continue;
        case OP_NOISE: if (int e = noise_stage(src, dst, B, Hout, Wout, d.noise, st)) return e; continue;
        case OP_JPEG: if (int e = jpeg_stage(src, dst, ws + p.planes_at, B, Hout, Wout, d.jpeg, st)) return e; continue;
        case OP_TONE: if (int e = tone_stage(src, dst, ws + p.tone_at, B, Hout, Wout, d.tone, st)) return e; continue;
        case OP_LSUM:
            hipLaunchKernelGGL(k_jitter_lsum, l.grid, block, 0, st, src, (int64_t)Hout * Wout, d.jitter_order, d.jitter_factors, sums);
            break;
        case OP_JITTER_NORM:
            hipLaunchKernelGGL(k_jitter_norm, l.grid, block, 0, st, src, d.out, Hout, Wout, d.jitter_order, d.jitter_factors, sums, d.flips, m0, m1, m2,
                               s0, s1, s2, B);
            break;
        case OP_U8_NORM: hipLaunchKernelGGL(k_u8_norm, l.grid, block, 0, st, src, d.out, Hout, Wout, d.flips, m0, m1, m2, s0, s1, s2, B); break;
        }
        SD_LAUNCH_CHECK();
    }
    return 0;
}

// plan + the checks of the workspace + launcher, under the caller's name
static int run_chain(const char* what, const sd_preprocess_desc* d, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    ChainPlan p;
    if (int e = plan_chain(d, what, &p)) return e;
    SD_REQUIRE(workspace, SD_ERR_INVALID, "%s: null pointer (workspace)", what);
    SD_REQUIRE(aligned16(workspace) || !(d->jpeg || d->tone), SD_ERR_INVALID, "%s: jpeg and tone need a 16-byte aligned workspace", what);
    SD_REQUIRE(workspace_bytes >= p.ws_bytes, SD_ERR_WORKSPACE, "%s: workspace %zu < %zu", what, workspace_bytes, p.ws_bytes);
    return launch_chain(*d, p, reinterpret_cast<uint8_t*>(workspace), (hipStream_t)stream);
}

size_t sd_preprocess_chain_workspace_bytes(const sd_preprocess_desc* d) {
    ChainPlan p;
    return plan_chain(d, "sd_preprocess_chain_workspace_bytes", &p) ? 0 : p.ws_bytes;
}

int sd_preprocess_chain(const sd_preprocess_desc* d, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    return run_chain("sd_preprocess_chain", d, workspace, workspace_bytes, stream);
}

const char* sd_preprocess_kernel_names(const sd_preprocess_desc* d) {
    static thread_local char line[1536];
    static const char* const buffers[] = {"tmp", "A", "B", "out", "sums"};
    ChainPlan p;
    if (plan_chain(d, "sd_preprocess_kernel_names", &p)) {
        snprintf(line, sizeof(line), "refused: %s", sd_last_error());
        return line;
    }
    int at = 0;
    for (int i = 0; i < p.n && (size_t)at < sizeof(line); ++i) {
        const ChainStep& s = p.steps[i];
        const char* sep = i ? "; " : "";
        if (s.op == OP_MEMSET || (s.op >= OP_BLUR && s.op <= OP_TONE)) {
            at += snprintf(line + at, sizeof(line) - at, "%s%s", sep, chain_name(*d, s));
            continue;
        }
        const ChainDims l = chain_dims(*d, p, s.op);
        at += snprintf(line + at, sizeof(line) - at, "%s%s grid=%ux%ux%u block=256 lds=%zu dst=%s", sep, chain_name(*d, s), l.grid.x, l.grid.y,
                       l.grid.z, l.lds, buffers[s.dst]);
    }
    return line;
}

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

// ---- the legacy entry points: each fills a descriptor and runs the chain under its own name -----------------------------------------
// Their arguments carry the names of the descriptor's fields, so the macros below copy them by name; a form has no slot for the stages
// that came after it, which stay null.  What a form asks beyond the chain (the table it is named after) is checked in its body.
#define SD_DESC_RESIZE(LIST)                                                                                                               \
    sd_preprocess_desc d = {};                                                                                                             \
    d.images = images; d.list = LIST; d.B = B; d.Hin = Hin; d.Win = Win; d.Hout = Hout; d.Wout = Wout; d.h_bounds = h_bounds; d.h_kk = h_kk; \
    d.h_ksize = h_ksize; d.v_bounds = v_bounds; d.v_kk = v_kk; d.v_ksize = v_ksize; d.flips = flips; d.mean3 = mean3; d.std3 = std3; d.out = out
#define SD_DESC_JITTER d.jitter_order = jitter_order; d.jitter_factors = jitter_factors
#define SD_DESC_STAGES SD_DESC_JITTER; d.affine = affine; d.mosaic_geom = mosaic_geom; d.mosaic_affine = mosaic_affine; d.fill3 = fill3
#define SD_DESC_GEOMETRY d.geometry = geometry; d.Hg = Hg; d.Wg = Wg; d.g0 = g0; d.g1 = g1; d.window = window
#define SD_RUN_CHAIN return run_chain(__func__, &d, workspace, workspace_bytes, stream)

int sd_preprocess_images(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                         int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const float* mean3,
                         const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0);
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                              int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const float* mean3,
                              const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1);
    SD_RUN_CHAIN;
}

int sd_preprocess_images_jitter(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const float* mean3, const float* std3, float* out, void* workspace,
                                size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_JITTER;
    SD_REQUIRE(jitter_order && jitter_factors, SD_ERR_INVALID, "%s: null jitter parameters", __func__);
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_jitter(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                     int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                     const float* jitter_factors, const float* mean3, const float* std3, float* out, void* workspace,
                                     size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_JITTER;
    SD_REQUIRE(jitter_order && jitter_factors, SD_ERR_INVALID, "%s: null jitter parameters", __func__);
    SD_RUN_CHAIN;
}

int sd_preprocess_images_affine(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const double* affine, const uint8_t* fill3, const float* mean3, const float* std3,
                                float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_JITTER; d.affine = affine; d.fill3 = fill3;
    SD_REQUIRE(affine && fill3, SD_ERR_INVALID, "%s: null affine matrices or fill colour", __func__);
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_affine(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                     const int* jitter_order, const float* jitter_factors, const double* affine, const uint8_t* fill3,
                                     const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                     sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_JITTER; d.affine = affine; d.fill3 = fill3;
    SD_REQUIRE(affine && fill3, SD_ERR_INVALID, "%s: null affine matrices or fill colour", __func__);
    SD_RUN_CHAIN;
}

int sd_preprocess_images_mosaic(const uint8_t* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds, const int* h_kk,
                                int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips, const int* jitter_order,
                                const float* jitter_factors, const double* affine, const int* mosaic_geom, const double* mosaic_affine,
                                const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_STAGES;
    SD_REQUIRE(mosaic_geom && mosaic_affine && fill3, SD_ERR_INVALID, "%s: null mosaic tables or fill colour", __func__);
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_mosaic(const uint8_t* const* images, int B, int Hin, int Win, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const uint8_t* flips,
                                     const int* jitter_order, const float* jitter_factors, const double* affine, const int* mosaic_geom,
                                     const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                                     void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_STAGES;
    SD_REQUIRE(mosaic_geom && mosaic_affine && fill3, SD_ERR_INVALID, "%s: null mosaic tables or fill colour", __func__);
    SD_RUN_CHAIN;
}

int sd_preprocess_images_window(const uint8_t* images, int B, int Hin, int Win, int Hc, int Wc, int Hout, int Wout, const int* h_bounds,
                                const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const int* window, int max_rows,
                                int max_cols, const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3,
                                float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_STAGES;
    d.geometry = SD_GEOM_WINDOW; d.Hg = Hc; d.Wg = Wc; d.g0 = max_rows; d.g1 = max_cols; d.window = window;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_window(const uint8_t* const* images, int B, int Hin, int Win, int Hc, int Wc, int Hout, int Wout, const int* h_bounds,
                                     const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize, const int* window,
                                     int max_rows, int max_cols, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                     const double* affine, const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3,
                                     const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                                     sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_STAGES;
    d.geometry = SD_GEOM_WINDOW; d.Hg = Hc; d.Wg = Wc; d.g0 = max_rows; d.g1 = max_cols; d.window = window;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_letterbox(const uint8_t* images, int B, int Hin, int Win, int Hi, int Wi, int Hout, int Wout, int y0, int x0,
                                   const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                                   const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                   const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3, const float* mean3, const float* std3,
                                   float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_STAGES;
    d.geometry = SD_GEOM_LETTERBOX; d.Hg = Hi; d.Wg = Wi; d.g0 = y0; d.g1 = x0;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_letterbox(const uint8_t* const* images, int B, int Hin, int Win, int Hi, int Wi, int Hout, int Wout, int y0, int x0,
                                        const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                                        const uint8_t* flips, const int* jitter_order, const float* jitter_factors, const double* affine,
                                        const int* mosaic_geom, const double* mosaic_affine, const uint8_t* fill3, const float* mean3,
                                        const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_STAGES;
    d.geometry = SD_GEOM_LETTERBOX; d.Hg = Hi; d.Wg = Wi; d.g0 = y0; d.g1 = x0;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_blur(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const int* mosaic_geom, const double* mosaic_affine, const int* blur, const uint8_t* fill3,
                              const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.blur = blur;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_blur(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const int* mosaic_geom, const double* mosaic_affine, const int* blur, const uint8_t* fill3,
                                   const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.blur = blur;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_persp(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                               const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                               const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                               const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                               const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace, size_t workspace_bytes,
                               sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.persp = persp; d.blur = blur;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_persp(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                    int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                    int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                    const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                    const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace,
                                    size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.persp = persp; d.blur = blur;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_jpeg(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                              const int* jpeg, const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace,
                              size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.persp = persp; d.blur = blur; d.jpeg = jpeg;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_jpeg(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                   const int* jpeg, const uint8_t* fill3, const float* mean3, const float* std3, float* out, void* workspace,
                                   size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.persp = persp; d.blur = blur; d.jpeg = jpeg;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_tone(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                              const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                              const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                              const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                              const int* jpeg, const int* tone, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                              void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.persp = persp; d.blur = blur; d.jpeg = jpeg; d.tone = tone;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_tone(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                   int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                   int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                   const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                   const int* jpeg, const int* tone, const uint8_t* fill3, const float* mean3, const float* std3, float* out,
                                   void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.persp = persp; d.blur = blur; d.jpeg = jpeg; d.tone = tone;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_noise(const uint8_t* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout, int g0, int g1,
                               const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk, int v_ksize,
                               const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                               const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                               const int* jpeg, const int* tone, const int* noise, const uint8_t* fill3, const float* mean3, const float* std3,
                               float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(0); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.persp = persp; d.blur = blur; d.jpeg = jpeg; d.tone = tone; d.noise = noise;
    SD_RUN_CHAIN;
}

int sd_preprocess_images_list_noise(const uint8_t* const* images, int geometry, int B, int Hin, int Win, int Hg, int Wg, int Hout, int Wout,
                                    int g0, int g1, const int* h_bounds, const int* h_kk, int h_ksize, const int* v_bounds, const int* v_kk,
                                    int v_ksize, const int* window, const uint8_t* flips, const int* jitter_order, const float* jitter_factors,
                                    const double* affine, const double* persp, const int* mosaic_geom, const double* mosaic_affine, const int* blur,
                                    const int* jpeg, const int* tone, const int* noise, const uint8_t* fill3, const float* mean3, const float* std3,
                                    float* out, void* workspace, size_t workspace_bytes, sd_stream_t stream) {
    SD_DESC_RESIZE(1); SD_DESC_GEOMETRY; SD_DESC_STAGES; d.persp = persp; d.blur = blur; d.jpeg = jpeg; d.tone = tone; d.noise = noise;
    SD_RUN_CHAIN;
}

}  // extern "C"

