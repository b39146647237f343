// What every kernel file shares: the export macro, the block size, the native
// 16-B vector and the bf16 conversions.  One definition each: pack2 and f2bf
// are the rounding (to nearest even) that the bit-exact suites hold every
// kernel to.  All of it is __forceinline__ in an anonymous namespace: each
// .hip file is its own translation unit of one shared library, and nothing
// here becomes a symbol.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VGPU_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr int kThreads = 256;  // workgroup size (4 waves) of every kernel that does not name its own

// Native 16-B vector (HIP's uint4 is a class; copies of it go through memcpy
// and defeat register promotion of staging arrays).
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
// v_cvt_pk_bf16_f32 on gfx950 (round-to-nearest-even, NaN-preserving)
__device__ __forceinline__ uint16_t f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(uint16_t, b);
}

// 8 bf16 in a 16-B vector (memory order) -> f[0..7].  A pointer, not an array
// of 8: gemv_fp8.hip fills the halves of a 16-float row.
__device__ __forceinline__ void unpack8(const u32x4 v, float* f) {
  f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
  f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
  f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
// One v_cvt_pk_bf16_f32 per pair (the same rounding as two scalar
// conversions, which cost two conversions + shift + or).
__device__ __forceinline__ uint32_t pack2(float lo, float hi) {
  typedef __attribute__((ext_vector_type(2))) float f2;
  typedef __attribute__((ext_vector_type(2))) __bf16 b2;
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f2{lo, hi}, b2));
}
__device__ __forceinline__ u32x4 pack8(const float (&f)[8]) {
  return u32x4{pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7])};
}

// 8 fp32 as two 16-B accesses
__device__ __forceinline__ void load8f(const float* p, float (&f)[8]) {
  const float4 a = reinterpret_cast<const float4*>(p)[0], b = reinterpret_cast<const float4*>(p)[1];
  f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
  f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
}
__device__ __forceinline__ void store8f(float* p, const float (&f)[8]) {
  reinterpret_cast<float4*>(p)[0] = float4{f[0], f[1], f[2], f[3]};
  reinterpret_cast<float4*>(p)[1] = float4{f[4], f[5], f[6], f[7]};
}

// Sum over the 64 lanes of a wave, the same in every lane.
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

}  // namespace
