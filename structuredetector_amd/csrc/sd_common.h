// Shared host/device helpers for libsdnet_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "../../include/sdnet_hip.h"

namespace sd {

void set_error(const char* fmt, ...);

#define SD_REQUIRE(cond, code, ...)            \
    do {                                       \
        if (!(cond)) {                         \
            sd::set_error(__VA_ARGS__);        \
            return (code);                     \
        }                                      \
    } while (0)

#define SD_HIP(call)                                                                    \
    do {                                                                                \
        hipError_t e_ = (call);                                                         \
        if (e_ != hipSuccess) {                                                         \
            sd::set_error("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (int)e_;                                                             \
        }                                                                               \
    } while (0)

#define SD_LAUNCH_CHECK()                                                               \
    do {                                                                                \
        hipError_t e_ = hipGetLastError();                                              \
        if (e_ != hipSuccess) {                                                         \
            sd::set_error("kernel launch failed: %s (%s:%d)", hipGetErrorString(e_), __FILE__, __LINE__); \
            return (int)e_;                                                             \
        }                                                                               \
    } while (0)

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

constexpr float kClampLo = 1e-6f;                    // fp32(1e-6)
constexpr float kClampHi = (float)(1.0 - 1e-6);      // fp32(1-1e-6) = 0.99999898672

// clamp(sigmoid(x), 1e-6, 1-1e-6): src/sdnet/utils/utils.py:355-361
__device__ __forceinline__ float sigmoid_raw(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float clamped_sigmoid(float x) {
    return fminf(fmaxf(sigmoid_raw(x), kClampLo), kClampHi);
}

// bf16 <-> fp32 (round to nearest even: v_cvt_pk_bf16_f32) and four-element activation accessors used by the kernels that exist
// for both activation types (fp32, and bf16 for the mixed-precision training path: i indexes groups of four elements)
__device__ __forceinline__ float bf16_to_f32(uint16_t v) { return __uint_as_float((uint32_t)v << 16); }
__device__ __forceinline__ uint16_t f32_to_bf16(float v) { return __builtin_bit_cast(uint16_t, (__bf16)v); }
// (activation streams of the HBM-bound passes are read ONCE: non-temporal loads -- `global_load_dwordx4 ... nt` -- keep them from displacing
//  what the next kernel re-reads; same-box A/B: fp32 step -0.7 %, mixed-precision step -0.6 %; non-temporal STORES changed nothing)
typedef float sd_f32x4_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p, int64_t i) {
    const sd_f32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const sd_f32x4_nt*>(p) + i);
    return make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ float4 ld4(const uint16_t* p, int64_t i) {
    const uint2 r = reinterpret_cast<const uint2*>(p)[i];
    return make_float4(bf16_to_f32((uint16_t)(r.x & 0xffff)), bf16_to_f32((uint16_t)(r.x >> 16)), bf16_to_f32((uint16_t)(r.y & 0xffff)),
                       bf16_to_f32((uint16_t)(r.y >> 16)));
}
__device__ __forceinline__ void st4(float* p, int64_t i, const float4 v) { reinterpret_cast<float4*>(p)[i] = v; }
__device__ __forceinline__ void st4(uint16_t* p, int64_t i, const float4 v) {
    uint2 pk;
    pk.x = (uint32_t)f32_to_bf16(v.x) | ((uint32_t)f32_to_bf16(v.y) << 16);
    pk.y = (uint32_t)f32_to_bf16(v.z) | ((uint32_t)f32_to_bf16(v.w) << 16);
    reinterpret_cast<uint2*>(p)[i] = pk;
}

// Head (1x1 conv C -> Co): Co <= HEAD_NARROW_MAX_CO takes the kernels of sd_nn.hip; wider heads (up to SD_HEAD_MAX_CO, C in {64, 128, 256})
// the GEMM kernels of sd_head_wide.hip, reached through the sd_head_* entry points of sd_nn.hip.
constexpr int HEAD_NARROW_MAX_CO = 32;
int head_wide_check(const char* fn, int64_t P, int C, int Co);                       // 0, or SD_ERR_INVALID with the message set
int head_wide_fwd(const float* x, const float* w, const float* bias, float* y, int B, int HW, int C, int Co, hipStream_t st);
int head_wide_fwd_bf16(const void* x, const float* w, const float* bias, float* y, int B, int HW, int C, int Co, hipStream_t st);
size_t head_wide_bwd_workspace_bytes(int64_t P, int C, int Co);
// weight / bias gradient partial rows (rows x (Co * C + Co) floats, finished by the caller in a fixed order), and the data gradient
int head_wide_wgrad(const float* dy, const float* x, float* partial, int B, int HW, int C, int Co, hipStream_t st, int& rows);
int head_wide_dgrad(const float* dy, const float* w, float* dx, int B, int HW, int C, int Co, hipStream_t st);

// Gaussian blur stage (sd_blur.hip): in -> mid -> out, each (B, H, W, 3) u8; mid differs from in and out, out may be in.  blur (B, 3)
// int32 on the device.  Shapes are the caller's to check (B and cdiv(H, 64) are grid dimensions: <= 65535).
int blur_stage(const uint8_t* in, uint8_t* mid, uint8_t* out, int B, int H, int W, const int* blur, hipStream_t st);

// JPEG round-trip stage (sd_jpeg.hip): in -> planes -> out, in and out (B, H, W, 3) u8 with H and W multiples of 16, out may be in.
// planes: jpeg_planes_bytes() bytes, 16-byte aligned.  table (B, 129) int32 on the device.  Shapes are the caller's to check (B and
// cdiv(H, 64) are grid dimensions: <= 65535).
size_t jpeg_planes_bytes(int B, int H, int W);
int jpeg_stage(const uint8_t* in, uint8_t* out, uint8_t* planes, int B, int H, int W, const int* table, hipStream_t st);

// Histogram tone stage (sd_tone.hip): in -> out, (B, H, W, 3) u8 of any alignment, out may be in.  ws: tone_workspace_bytes() bytes,
// 16-byte aligned.  table (B, 4) int32 on the device.  Shapes are the caller's to check (B is a grid dimension: <= 65535; H W < 2^31).
size_t tone_workspace_bytes(int B);
int tone_stage(const uint8_t* in, uint8_t* out, void* ws, int B, int H, int W, const int* table, hipStream_t st);

// Sensor noise stage (sd_noise.hip): in -> out, (B, H, W, 3) u8 of any alignment, out may be in.  No workspace.  table (B, 4) int32 on
// the device.  Shapes are the caller's to check (B is a grid dimension: <= 65535; H W < 2^31).
int noise_stage(const uint8_t* in, uint8_t* out, int B, int H, int W, const int* table, hipStream_t st);

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

}  // namespace sd
