// One Llama decode step (batch ≤ 8, one new token per row) between the skinny
// GEMVs of skinny.hip: residual add + RMSNorm, RoPE + KV-cache write,
// single-query grouped-query attention over the cache, SwiGLU.
//
//   add_rmsnorm     h = bf16(x + delta) -> x;  y = bf16(h·rsqrt(mean(h²)+eps)·w)
//   rope_kv_write   q, k rotated (half-split pairs) from the wqkv row; k, v
//                   stored at row *pos of the [B][KVH][ctx][hd] caches
//   attn_decode     softmax(q·Kᵀ·scale)·V over keys 0..*pos, split over key
//                   chunks: partial (m, l, o) per (row, head, chunk) into ws,
//                   merged in chunk order by a second launch
//   swiglu          y = bf16(silu(g)·u) from [g | u]
//
// A token is 16 GB of weights through the GEMVs; everything here is a few MB
// per layer and latency-bound, so the kernels are sized for few, short
// dispatches: 16-B loads, fp32 math, one rounding to bf16 at each output.
// `pos` is a device int64 read by the kernels, so a captured graph replays at
// any position; grids depend on shapes only.  No atomics, no hand-off between
// workgroups inside a launch: the same inputs give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16.h"

namespace {

// exp(a - b) for softmax maxima: 0 when a is the empty maximum (-inf), also
// when b is (-inf - -inf would be NaN).
__device__ __forceinline__ float exp_diff(float a, float b) { return a == -INFINITY ? 0.0f : __expf(a - b); }

// ---- residual add + RMSNorm: a block per row, thread = 8 columns per pass ------------
// Pass 1 forms h (written back to x when there is a delta) and Σh²; pass 2
// reads h back (the thread's own stores, or x itself) and scales it.
__global__ void __launch_bounds__(kThreads) add_rmsnorm_kernel(uint16_t* __restrict__ x,
                                                               const uint16_t* __restrict__ delta,
                                                               const uint16_t* __restrict__ w,
                                                               uint16_t* __restrict__ y, int dim, float eps) {
  __shared__ float part[kThreads / 64];
  const int kv = dim >> 3;
  u32x4* X = reinterpret_cast<u32x4*>(x + (int64_t)blockIdx.x * dim);
  const u32x4* D = delta ? reinterpret_cast<const u32x4*>(delta + (int64_t)blockIdx.x * dim) : nullptr;
  float ss = 0.0f;
  for (int c = threadIdx.x; c < kv; c += kThreads) {
    float h[8];
    unpack8(X[c], h);
    if (D) {
      float d[8];
      unpack8(D[c], d);
#pragma unroll
      for (int j = 0; j < 8; ++j) h[j] += d[j];
      const u32x4 hv = pack8(h);
      X[c] = hv;
      unpack8(hv, h);  // the norm sees the rounded residual
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) ss = fmaf(h[j], h[j], ss);
  }
  ss = wave_sum(ss);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  ss = 0.0f;
#pragma unroll
  for (int q = 0; q < kThreads / 64; ++q) ss += part[q];  // fixed order
  const float r = 1.0f / sqrtf(ss / (float)dim + eps);
  const u32x4* W = reinterpret_cast<const u32x4*>(w);
  u32x4* Y = reinterpret_cast<u32x4*>(y + (int64_t)blockIdx.x * dim);
  for (int c = threadIdx.x; c < kv; c += kThreads) {
    float h[8], g[8];
    unpack8(X[c], h);
    unpack8(W[c], g);
#pragma unroll
    for (int j = 0; j < 8; ++j) h[j] = h[j] * r * g[j];
    Y[c] = pack8(h);
  }
}

// ---- RoPE + cache write: thread = 8 columns of a head's first half and the 8
// they pair with in its second half.  Heads 0..H-1 are q, then KVH of k, then
// KVH of v (copied as they are).
__global__ void __launch_bounds__(kThreads) rope_kv_write_kernel(const uint16_t* __restrict__ qkv,
                                                                 const float* __restrict__ cos_t,
                                                                 const float* __restrict__ sin_t,
                                                                 const int64_t* __restrict__ pos,
                                                                 uint16_t* __restrict__ q_out,
                                                                 uint16_t* __restrict__ kcache,
                                                                 uint16_t* __restrict__ vcache, int B, int H,
                                                                 int KVH, int hd, int ctx, int max_seq) {
  const int per_head = hd >> 4, heads = H + 2 * KVH;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= B * heads * per_head) return;
  const int64_t p = *pos;
  if (p < 0 || p >= ctx || p >= max_seq) return;  // no table row, no cache row: nothing is written
  const int c = i % per_head, head = (i / per_head) % heads, b = i / (per_head * heads);
  const int half = hd >> 1;
  const uint16_t* src = qkv + ((int64_t)b * heads + head) * hd + c * 8;
  const u32x4 v1 = *reinterpret_cast<const u32x4*>(src), v2 = *reinterpret_cast<const u32x4*>(src + half);
  uint16_t* dst;
  if (head < H) {
    dst = q_out + ((int64_t)b * H + head) * hd;
  } else {
    const int kh = head < H + KVH ? head - H : head - H - KVH;
    dst = (head < H + KVH ? kcache : vcache) + (((int64_t)b * KVH + kh) * ctx + p) * hd;
  }
  dst += c * 8;
  if (head >= H + KVH) {
    *reinterpret_cast<u32x4*>(dst) = v1;
    *reinterpret_cast<u32x4*>(dst + half) = v2;
    return;
  }
  float x1[8], x2[8], cs[8], sn[8], o1[8], o2[8];
  unpack8(v1, x1);
  unpack8(v2, x2);
  load8f(cos_t + p * half + c * 8, cs);
  load8f(sin_t + p * half + c * 8, sn);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    o1[j] = x1[j] * cs[j] - x2[j] * sn[j];
    o2[j] = x1[j] * sn[j] + x2[j] * cs[j];
  }
  *reinterpret_cast<u32x4*>(dst) = pack8(o1);
  *reinterpret_cast<u32x4*>(dst + half) = pack8(o2);
}

// ---- attention over the cache, one query row per head ------------------------------
// Block = (key chunk, kv head, batch row), its G = H/KVH query heads in
// registers so that every K and V load serves all of them.  A key row is L =
// hd/8 lanes of 16 B; the S = 64/L lane groups of a wave take S consecutive
// keys, kAttnU such sets in flight per wave per trip.  Each lane group runs
// its own online softmax (fp32 running max m, sum l, o over the lane's 8
// columns); the groups of a wave meet through shuffles, the 4 waves through
// LDS in wave order.  Keys beyond *pos are neither loaded nor counted; a chunk
// wholly beyond it stores the empty partial (m = -inf, l = 0, o = 0).
constexpr int kAttnU = 4;
constexpr int kAttnWaves = kThreads / 64;
constexpr int kChunkKeys = 128;    // keys per block (32 per wave: two trips at hd = 128)
constexpr int kMaxChunks = 64;     // beyond 8192 keys the chunks grow instead
constexpr int kWsHead = 4;         // floats in front of o in a partial: m, l, two unused (keeps o 16-B aligned)

inline int attn_chunk(int ctx) {
  if (ctx <= kChunkKeys * kMaxChunks) return kChunkKeys;
  const int per = (ctx + kMaxChunks - 1) / kMaxChunks;
  return (per + 63) / 64 * 64;
}

template <int HD, int G>
__global__ void __launch_bounds__(kThreads) attn_decode_partial_kernel(const uint16_t* __restrict__ q,
                                                                       const uint16_t* __restrict__ kcache,
                                                                       const uint16_t* __restrict__ vcache,
                                                                       const int64_t* __restrict__ pos,
                                                                       float* __restrict__ ws, int H, int KVH,
                                                                       int ctx, int chunk, float scale) {
  constexpr int L = HD / 8, S = 64 / L, U = kAttnU;
  __shared__ float sm[kAttnWaves][G][HD + 2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane % L, slot = lane / L;
  const int ck = blockIdx.x, kh = blockIdx.y, b = blockIdx.z;
  const int64_t p = *pos;
  const int n = p < 0 ? 0 : (p + 1 < (int64_t)ctx ? (int)(p + 1) : ctx);  // keys 0..n-1 count
  const int k0 = ck * chunk;
  const int k1 = k0 + chunk < n ? k0 + chunk : n;

  float qf[G][8], o[G][8], m[G], l[G];
#pragma unroll
  for (int g = 0; g < G; ++g) {
    unpack8(reinterpret_cast<const u32x4*>(q + ((int64_t)b * H + kh * G + g) * HD)[j], qf[g]);
    m[g] = -INFINITY;
    l[g] = 0.0f;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      qf[g][d] *= scale;
      o[g][d] = 0.0f;
    }
  }
  const int64_t row0 = ((int64_t)b * KVH + kh) * ctx;
  const u32x4* K = reinterpret_cast<const u32x4*>(kcache) + row0 * L + j;
  const u32x4* V = reinterpret_cast<const u32x4*>(vcache) + row0 * L + j;

  for (int kb = k0 + wave * (U * S); kb < k1; kb += kAttnWaves * U * S) {
    u32x4 kv[U], vv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int key = kb + u * S + slot;
      const bool ok = key < k1;
      kv[u] = ok ? K[(int64_t)key * L] : u32x4{0u, 0u, 0u, 0u};
      vv[u] = ok ? V[(int64_t)key * L] : u32x4{0u, 0u, 0u, 0u};
    }
    float s[G][U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float kf[8];
      unpack8(kv[u], kf);
      const bool ok = kb + u * S + slot < k1;
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float a = 0.0f;
#pragma unroll
        for (int d = 0; d < 8; ++d) a = fmaf(qf[g][d], kf[d], a);
#pragma unroll
        for (int off = 1; off < L; off <<= 1) a += __shfl_xor(a, off, 64);
        s[g][u] = ok ? a : -INFINITY;
      }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
      float mx = m[g];
#pragma unroll
      for (int u = 0; u < U; ++u) mx = fmaxf(mx, s[g][u]);
      const float alpha = exp_diff(m[g], mx);
      m[g] = mx;
      float ls = l[g] * alpha;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        s[g][u] = exp_diff(s[g][u], mx);  // the probability from here on
        ls += s[g][u];
      }
      l[g] = ls;
#pragma unroll
      for (int d = 0; d < 8; ++d) o[g][d] *= alpha;
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      float vf[8];
      unpack8(vv[u], vf);
#pragma unroll
      for (int g = 0; g < G; ++g)
#pragma unroll
        for (int d = 0; d < 8; ++d) o[g][d] = fmaf(s[g][u], vf[d], o[g][d]);
    }
  }

  // the S lane groups of the wave
#pragma unroll
  for (int off = L; off < 64; off <<= 1) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const float m2 = __shfl_xor(m[g], off, 64), l2 = __shfl_xor(l[g], off, 64);
      const float mx = fmaxf(m[g], m2);
      const float a1 = exp_diff(m[g], mx), a2 = exp_diff(m2, mx);
      m[g] = mx;
      l[g] = l[g] * a1 + l2 * a2;
#pragma unroll
      for (int d = 0; d < 8; ++d) o[g][d] = o[g][d] * a1 + __shfl_xor(o[g][d], off, 64) * a2;
    }
  }
  if (slot == 0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (j == 0) {
        sm[wave][g][0] = m[g];
        sm[wave][g][1] = l[g];
      }
#pragma unroll
      for (int d = 0; d < 8; ++d) sm[wave][g][2 + j * 8 + d] = o[g][d];
    }
  }
  __syncthreads();
  // the 4 waves, in wave order: thread = (head g, 8 columns)
  if (threadIdx.x < G * L) {
    const int g = threadIdx.x / L, jj = threadIdx.x % L;
    float mx = -INFINITY;
#pragma unroll
    for (int w = 0; w < kAttnWaves; ++w) mx = fmaxf(mx, sm[w][g][0]);
    float ls = 0.0f, acc[8] = {};
#pragma unroll
    for (int w = 0; w < kAttnWaves; ++w) {
      const float a = exp_diff(sm[w][g][0], mx);
      ls = fmaf(sm[w][g][1], a, ls);
#pragma unroll
      for (int d = 0; d < 8; ++d) acc[d] = fmaf(sm[w][g][2 + jj * 8 + d], a, acc[d]);
    }
    float* out = ws + (((int64_t)b * H + kh * G + g) * gridDim.x + ck) * (HD + kWsHead);
    if (jj == 0) {
      out[0] = mx;
      out[1] = ls;
    }
    store8f(out + kWsHead + jj * 8, acc);
  }
}

// out[b][h][:] = bf16(Σ_c o_c·e^(m_c - M) / Σ_c l_c·e^(m_c - M)), chunks in order;
// thread = 8 columns of one (row, head).  No key at all (*pos < 0): zeros.
__global__ void __launch_bounds__(kThreads) attn_decode_combine_kernel(const float* __restrict__ ws,
                                                                       uint16_t* __restrict__ out, int total,
                                                                       int hd, int chunks) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const int L = hd >> 3, bh = i / L, j = i % L;
  const int stride = hd + kWsHead;
  const float* base = ws + (int64_t)bh * chunks * stride;
  float mx = -INFINITY;
  for (int c = 0; c < chunks; ++c) mx = fmaxf(mx, base[(int64_t)c * stride]);
  float ls = 0.0f, acc[8] = {};
  for (int c = 0; c < chunks; ++c) {
    const float* pc = base + (int64_t)c * stride;
    const float mc = pc[0];
    if (mc == -INFINITY) continue;  // an empty chunk
    const float a = __expf(mc - mx);
    float oc[8];
    load8f(pc + kWsHead + j * 8, oc);
    ls = fmaf(pc[1], a, ls);
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] = fmaf(oc[d], a, acc[d]);
  }
  if (ls > 0.0f) {
#pragma unroll
    for (int d = 0; d < 8; ++d) acc[d] /= ls;
  }
  reinterpret_cast<u32x4*>(out)[(int64_t)bh * L + j] = pack8(acc);
}

// ---- SwiGLU: thread = 8 columns of one row -----------------------------------------
__global__ void __launch_bounds__(kThreads) swiglu_kernel(const uint16_t* __restrict__ gu,
                                                          uint16_t* __restrict__ y, int total8, int ffn8) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= total8) return;
  const int b = i / ffn8, c = i % ffn8;
  const u32x4* row = reinterpret_cast<const u32x4*>(gu) + (int64_t)b * 2 * ffn8;
  float g[8], u[8];
  unpack8(row[c], g);
  unpack8(row[ffn8 + c], u);
#pragma unroll
  for (int j = 0; j < 8; ++j) g[j] = g[j] / (1.0f + expf(-g[j])) * u[j];
  reinterpret_cast<u32x4*>(y)[i] = pack8(g);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool batch_ok(int B) { return B == 1 || B == 2 || B == 3 || B == 4 || B == 8; }

}  // namespace

VGPU_API int vgpu_decode_supported(int B, int H, int KVH, int hd, int ctx) {
  return batch_ok(B) && (hd == 64 || hd == 128) && H > 0 && KVH > 0 && H % KVH == 0 && H / KVH <= 8 && ctx >= 1;
}

// x [rows][dim] += delta (delta may be null), y = RMSNorm(x)·w; all bf16, dim % 8 == 0.
VGPU_API int vgpu_add_rmsnorm(void* x, const void* delta, const void* w, void* y, int rows, int dim, float eps,
                              hipStream_t s) {
  if (rows < 1 || dim < 8 || dim % 8 || !x || !w || !y || !al16(x) || !al16(delta) || !al16(w) || !al16(y))
    return -1;
  hipLaunchKernelGGL(add_rmsnorm_kernel, dim3(rows), dim3(kThreads), 0, s, (uint16_t*)x, (const uint16_t*)delta,
                     (const uint16_t*)w, (uint16_t*)y, dim, eps);
  return (int)hipGetLastError();
}

// qkv [B][(H+2·KVH)·hd] bf16; cos, sin [max_seq][hd/2] fp32; pos: one device int64.
// q_out [B][H][hd]; caches [B][KVH][ctx][hd], row *pos written (k rotated, v as it is).
VGPU_API int vgpu_rope_kv_write(const void* qkv, const void* cos_t, const void* sin_t, const void* pos, void* q_out,
                                void* kcache, void* vcache, int B, int H, int KVH, int hd, int ctx, int max_seq,
                                hipStream_t s) {
  if (!vgpu_decode_supported(B, H, KVH, hd, ctx) || max_seq < 1 || !pos) return -1;
  if (!qkv || !cos_t || !sin_t || !q_out || !kcache || !vcache) return -1;
  if (!al16(qkv) || !al16(cos_t) || !al16(sin_t) || !al16(q_out) || !al16(kcache) || !al16(vcache)) return -1;
  const int items = B * (H + 2 * KVH) * (hd / 16);
  hipLaunchKernelGGL(rope_kv_write_kernel, dim3((items + kThreads - 1) / kThreads), dim3(kThreads), 0, s,
                     (const uint16_t*)qkv, (const float*)cos_t, (const float*)sin_t, (const int64_t*)pos,
                     (uint16_t*)q_out, (uint16_t*)kcache, (uint16_t*)vcache, B, H, KVH, hd, ctx, max_seq);
  return (int)hipGetLastError();
}

// Keys per block of vgpu_attn_decode: a function of ctx alone (the grid is frozen in a captured graph).
VGPU_API int vgpu_attn_decode_chunk(int ctx) { return ctx >= 1 ? attn_chunk(ctx) : -1; }

// Workspace (bytes) of vgpu_attn_decode: one fp32 (m, l, o[hd]) per (row, head, chunk).
VGPU_API int64_t vgpu_attn_decode_workspace(int B, int H, int hd, int ctx) {
  if (B < 1 || H < 1 || hd < 8 || ctx < 1) return -1;
  const int chunk = attn_chunk(ctx);
  return (int64_t)B * H * ((ctx + chunk - 1) / chunk) * (hd + kWsHead) * 4;
}

#define VGPU_ATTN_CASE(HD, G)                                                                                  \
  case G:                                                                                                      \
    hipLaunchKernelGGL((attn_decode_partial_kernel<HD, G>), grid, dim3(kThreads), 0, s, (const uint16_t*)q,    \
                       (const uint16_t*)kcache, (const uint16_t*)vcache, (const int64_t*)pos, (float*)ws, H,   \
                       KVH, ctx, chunk, scale);                                                                \
    break;
#define VGPU_ATTN_SWITCH(HD)                                                                                   \
  switch (H / KVH) {                                                                                           \
    VGPU_ATTN_CASE(HD, 1) VGPU_ATTN_CASE(HD, 2) VGPU_ATTN_CASE(HD, 3) VGPU_ATTN_CASE(HD, 4)                    \
    VGPU_ATTN_CASE(HD, 5) VGPU_ATTN_CASE(HD, 6) VGPU_ATTN_CASE(HD, 7) VGPU_ATTN_CASE(HD, 8)                    \
    default: return -1;                                                                                        \
  }

// out [B][H·hd] = attention of q [B][H][hd] over keys 0..*pos of the caches
// (query head h reads kv head h / (H/KVH)); two launches: partials, combine.
VGPU_API int vgpu_attn_decode(const void* q, const void* kcache, const void* vcache, const void* pos, void* out,
                              void* ws, int64_t ws_bytes, int B, int H, int KVH, int hd, int ctx, float scale,
                              hipStream_t s) {
  if (!vgpu_decode_supported(B, H, KVH, hd, ctx) || !q || !kcache || !vcache || !pos || !out || !ws) return -1;
  if (!al16(q) || !al16(kcache) || !al16(vcache) || !al16(out) || !al16(ws)) return -1;
  if (ws_bytes < vgpu_attn_decode_workspace(B, H, hd, ctx)) return -1;
  const int chunk = attn_chunk(ctx), chunks = (ctx + chunk - 1) / chunk;
  const dim3 grid(chunks, KVH, B);
  if (hd == 128) {
    VGPU_ATTN_SWITCH(128)
  } else {
    VGPU_ATTN_SWITCH(64)
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const int total = B * H * (hd / 8);
  hipLaunchKernelGGL(attn_decode_combine_kernel, dim3((total + kThreads - 1) / kThreads), dim3(kThreads), 0, s,
                     (const float*)ws, (uint16_t*)out, total, hd, chunks);
  return (int)hipGetLastError();
}

// y [B][ffn] = silu(g)·u from gu [B][2·ffn] = [g | u]; bf16, ffn % 8 == 0.
VGPU_API int vgpu_swiglu(const void* gu, void* y, int B, int ffn, hipStream_t s) {
  if (B < 1 || ffn < 8 || ffn % 8 || !gu || !y || !al16(gu) || !al16(y)) return -1;
  if ((int64_t)B * ffn / 8 > INT32_MAX) return -1;
  const int total8 = B * (ffn / 8);
  hipLaunchKernelGGL(swiglu_kernel, dim3((total8 + kThreads - 1) / kThreads), dim3(kThreads), 0, s,
                     (const uint16_t*)gu, (uint16_t*)y, total8, ffn / 8);
  return (int)hipGetLastError();
}
