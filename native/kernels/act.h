// The activation codes that the Python wrappers pass to every kernel file:
// 0 = none, 1 = relu, 2 = relu6.  act_fwd is the activation; act_grad is
// d act / dz as PyTorch defines it (threshold_backward / hardtanh_backward),
// which takes the pre-activation z or the stored output y alike: both are
// inside (0, 6) together.  <kAct> where the code is a template argument,
// (int, float) where it arrives in the kernel arguments.
#pragma once
#include <hip/hip_runtime.h>

namespace {

template <int kAct>
__device__ __forceinline__ float act_fwd(float z) {
  if constexpr (kAct == 1) return fmaxf(z, 0.0f);
  if constexpr (kAct == 2) return fminf(fmaxf(z, 0.0f), 6.0f);
  return z;
}
template <int kAct>
__device__ __forceinline__ float act_grad(float z) {
  if constexpr (kAct == 1) return z > 0.0f ? 1.0f : 0.0f;
  if constexpr (kAct == 2) return (z > 0.0f && z < 6.0f) ? 1.0f : 0.0f;
  return 1.0f;
}

__device__ __forceinline__ float act_fwd(int act, float z) {
  return act == 1 ? fmaxf(z, 0.0f) : act == 2 ? fminf(fmaxf(z, 0.0f), 6.0f) : z;
}
__device__ __forceinline__ float act_grad(int act, float z) {
  return act == 1 ? (z > 0.0f ? 1.0f : 0.0f) : act == 2 ? ((z > 0.0f && z < 6.0f) ? 1.0f : 0.0f) : 1.0f;
}

}  // namespace
