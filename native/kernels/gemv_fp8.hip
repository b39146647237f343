// Projection weights held as OCP fp8 (e4m3fn) codes with one fp32 scale per
// output row: the decode GEMV over them, and their expansion to bf16.
//
//   value of W[n][k] = scale[n] · e4m3(codes[n][k])          codes [N][K] uint8
//   gemv     y[b][n]  = bf16(scale[n] · Σ_k x[b][k] · e4m3(codes[n][k]))
//   dequant  out[n][k] = bf16(scale[n] · e4m3(codes[n][k]))
//
// The format is gfx950's own (v_cvt_pk_f32_fp8 decodes e4m3fn, bias 7, 0x7F /
// 0xFF NaN), not MI300X's fnuz.  A decode step is a stream over every weight
// (skinny.hip's forward kernel: 129 calls, 15.0 GB of bf16 per Llama-3-8B
// token); one byte per weight halves the stream.
//
// The GEMV is skinny_fwd_kernel's plan at one byte per weight: a block per kR
// output rows, its 4 waves splitting K in 16-byte chunks (16 weights against
// 32 B of x per batch row), kU chunks' loads in flight per lane, x unpacked
// once per chunk for all kR rows, fp32 accumulation, the waves' partials summed
// from LDS in wave order (bit-identical run to run), the scale applied once to
// the finished sum, one rounding to bf16.
//
// VALU per 16 weight bytes and lane: 8 packed converts + 16 B FMAs + 16 B / kR
// shifts or masks for x, against 8 + 8 B + 8 B / kR per 16 bytes of the bf16
// kernel.  What that costs at each batch size is measured in
// profiles/r9/fp8/README.md.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16.h"

namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 16;  // weights per 16-byte load
typedef __attribute__((ext_vector_type(2))) float f32x2;

// 16 e4m3 codes (memory order) -> 16 floats: two packed converts per 32-bit word
__device__ __forceinline__ void decode16(const u32x4 v, float (&f)[16]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], false);
    const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w[i], true);
    f[4 * i + 0] = lo.x; f[4 * i + 1] = lo.y; f[4 * i + 2] = hi.x; f[4 * i + 3] = hi.y;
  }
}

// Rows per block and chunks in flight per lane.  One trip of the K loop covers
// kThreads · kChunk · kU columns; see vgpu_gemv_fp8_trip.
// Four rows and one chunk: a row of K = 4096 is one chunk per thread, so the
// loads in flight per lane are the block's rows, and what a second chunk adds
// is registers (62 VGPRs at B = 1 against 108 for two chunks: 8 waves per SIMD
// against 4).  On MI355X over Llama-3-8B's shapes, weights walked from HBM
// (scripts/gemv_fp8_ab.py's method with each plan exported for the run, us per
// call at B = 1 / 8, the bf16 kernel beside it; profiles/r9/fp8/gemv_ab_plans.jsonl):
//                     4 x 1          4 x 2          8 x 1          2 x 4         bf16
//   6144 x 4096     7.3 /  31.1    8.0 /  56.1    8.9 /  39.5    9.1 /  65.2   10.2 /  37.5
//   4096 x 4096     6.1 /  21.9    6.1 /  38.1    7.4 /  22.7    7.0 /  44.2    7.9 /  26.3
//   28672 x 4096   21.8 / 130.0   26.1 / 252.9   24.1 / 139.3   32.6 / 297.7   39.0 / 161.0
//   4096 x 14336   14.1 /  36.7   13.6 /  59.8   16.8 /  46.7   13.6 /  74.7   22.3 /  51.0
// Two chunks win only the last shape at B = 1 and 2, by 4-7 %, and at B = 8
// (288 VGPRs, one wave per SIMD) lose to the bf16 kernel by 1.2-1.6 x.
constexpr int kRows = 4, kLoads = 1;

template <int B, int kR, int kU>
__global__ void __launch_bounds__(kThreads) gemv_fp8_kernel(const uint16_t* __restrict__ x,
                                                            const uint8_t* __restrict__ codes,
                                                            const float* __restrict__ scale,
                                                            uint16_t* __restrict__ y, int N, int K) {
  __shared__ float part[kWaves][kR * B];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * kR;
  float acc[kR][B];
#pragma unroll
  for (int r = 0; r < kR; ++r)
#pragma unroll
    for (int b = 0; b < B; ++b) acc[r][b] = 0.0f;
  const int kv = K / kChunk;  // 16-byte chunks per row of codes; a row of x holds 2 kv
  const u32x4* W[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r)  // a row past N reads row N - 1 (its sum is never stored)
    W[r] = reinterpret_cast<const u32x4*>(codes + (int64_t)min(n0 + r, N - 1) * K);
  const u32x4* X = reinterpret_cast<const u32x4*>(x);
  for (int c0 = wave * 64 + lane; c0 < kv; c0 += kThreads * kU) {
    u32x4 wv[kU][kR], xv[kU][B][2];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const int c = c0 + kThreads * u;
      if (c < kv) {
#pragma unroll
        for (int r = 0; r < kR; ++r) wv[u][r] = W[r][c];
#pragma unroll
        for (int b = 0; b < B; ++b) {
          xv[u][b][0] = X[(int64_t)b * 2 * kv + 2 * c];
          xv[u][b][1] = X[(int64_t)b * 2 * kv + 2 * c + 1];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      if (c0 + kThreads * u >= kv) continue;
      float xf[B][16];
#pragma unroll
      for (int b = 0; b < B; ++b) {
        unpack8(xv[u][b][0], xf[b]);
        unpack8(xv[u][b][1], xf[b] + 8);
      }
#pragma unroll
      for (int r = 0; r < kR; ++r) {
        float wf[16];
        decode16(wv[u][r], wf);
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
          for (int j = 0; j < 16; ++j) acc[r][b] = fmaf(wf[j], xf[b][j], acc[r][b]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < kR; ++r)
#pragma unroll
    for (int b = 0; b < B; ++b) {
      const float v = wave_sum(acc[r][b]);
      if (lane == 0) part[wave][r * B + b] = v;
    }
  __syncthreads();
  if (threadIdx.x < kR * B && n0 + (int)threadIdx.x / B < N) {  // thread (r, b) stores one output
    const int r = threadIdx.x / B, b = threadIdx.x % B;
    float v = 0.0f;
#pragma unroll
    for (int q = 0; q < kWaves; ++q) v += part[q][threadIdx.x];  // fixed order
    y[(int64_t)b * N + n0 + r] = f2bf(v * scale[n0 + r]);
  }
}

// One thread per 16 codes: a 16-byte load, two 16-byte stores.
__global__ void __launch_bounds__(kThreads) dequant_fp8_kernel(const uint8_t* __restrict__ codes,
                                                               const float* __restrict__ scale,
                                                               uint16_t* __restrict__ out, int64_t chunks, int kv) {
  const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= chunks) return;
  const float s = scale[i / kv];
  float f[16];
  decode16(reinterpret_cast<const u32x4*>(codes)[i], f);
#pragma unroll
  for (int j = 0; j < 16; ++j) f[j] *= s;
  u32x4* o = reinterpret_cast<u32x4*>(out) + 2 * i;
  o[0] = u32x4{pack2(f[0], f[1]), pack2(f[2], f[3]), pack2(f[4], f[5]), pack2(f[6], f[7])};
  o[1] = u32x4{pack2(f[8], f[9]), pack2(f[10], f[11]), pack2(f[12], f[13]), pack2(f[14], f[15])};
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

template <int kR, int kU>
int launch_gemv(const void* x, const void* codes, const void* scale, void* y, int B, int N, int K, hipStream_t s) {
  const dim3 grid((N + kR - 1) / kR);
#define VGPU_FP8_CASE(b)                                                                                       \
  case b:                                                                                                      \
    hipLaunchKernelGGL((gemv_fp8_kernel<b, kR, kU>), grid, dim3(kThreads), 0, s, (const uint16_t*)x,           \
                       (const uint8_t*)codes, (const float*)scale, (uint16_t*)y, N, K);                        \
    break;
  switch (B) {
    VGPU_FP8_CASE(1) VGPU_FP8_CASE(2) VGPU_FP8_CASE(3) VGPU_FP8_CASE(4) VGPU_FP8_CASE(8)
    default: return -1;
  }
#undef VGPU_FP8_CASE
  return (int)hipGetLastError();
}

}  // namespace

VGPU_API int vgpu_gemv_fp8_supported(int B, int N, int K) {
  return (B == 1 || B == 2 || B == 3 || B == 4 || B == 8) && N > 0 && K > 0 && N % 4 == 0 && K % kChunk == 0;
}

// Columns one trip of the kernel's K loop covers (tests place K either side of it).
VGPU_API int vgpu_gemv_fp8_trip() { return kThreads * kChunk * kLoads; }

// y [B][N] (bf16) = scale[n] · x [B][K] (bf16) · e4m3(codes [N][K])ᵀ; scale [N] fp32.
VGPU_API int vgpu_gemv_fp8(const void* x, const void* codes, const void* scale, void* y, int B, int N, int K,
                           hipStream_t s) {
  if (!x || !codes || !scale || !y || !vgpu_gemv_fp8_supported(B, N, K) || !al16(x) || !al16(codes)) return -1;
  return launch_gemv<kRows, kLoads>(x, codes, scale, y, B, N, K, s);
}

// out [N][K] (bf16) = scale[n] · e4m3(codes [N][K]).
VGPU_API int vgpu_dequant_fp8(const void* codes, const void* scale, void* out, int N, int K, hipStream_t s) {
  if (!codes || !scale || !out || N < 1 || K < kChunk || K % kChunk || !al16(codes) || !al16(out)) return -1;
  const int kv = K / kChunk;
  const int64_t chunks = (int64_t)N * kv;
  const int64_t blocks = (chunks + kThreads - 1) / kThreads;
  if (blocks > 0x7fffffff) return -1;
  hipLaunchKernelGGL(dequant_fp8_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, s, (const uint8_t*)codes,
                     (const float*)scale, (uint16_t*)out, chunks, kv);
  return (int)hipGetLastError();
}
