// Llama prefill: S prompt tokens at once into a KV cache that already holds
// `start` tokens, between the 1x1 GEMMs of conv_gemm.hip and the row kernels
// of decode.hip (add_rmsnorm and swiglu take any row count).
//
//   rope_kv_write_seq  q, k rotated (half-split pairs) from the wqkv rows; k, v
//                      stored at rows start .. start+S-1 of the
//                      [B][KVH][ctx][hd] caches, q to [B][S][H][hd]
//   attn_prefill       causal grouped-query flash attention on MFMA: row i of
//                      head h is softmax(q_i·Kᵀ·scale)·V over cache rows
//                      0 .. start+i of kv head h / (H/KVH), K and V read in
//                      place; out [B][S][H·hd] is token-major for the wo GEMM
//
// `start` is a host int: the grids and the key range depend on S and start, so
// a prefill launch is not replayed from a captured graph at other positions
// (decode.hip's kernels read `pos` on the device for that; these do not).
// fp32 math with one rounding to bf16 at each output (and of P into the PV
// MFMA), no atomics, no split over keys and no workspace: one workgroup owns
// its query tile for the whole key range, so the same inputs give the same
// bits whatever the grid.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16.h"

namespace {

typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;

// 2^(a - b) for softmax maxima and scores (both already in log2 units): 0 when
// a is -inf (a masked score, or the empty maximum), also when b is
// (-inf - -inf would be NaN).
__device__ __forceinline__ float exp2_diff(float a, float b) {
  return a == -INFINITY ? 0.0f : __builtin_amdgcn_exp2f(a - b);
}

// ---- RoPE + cache write for S tokens: thread = 8 columns of a head's first
// half and the 8 they pair with in its second half, of one token.  Heads
// 0..H-1 are q, then KVH of k, then KVH of v (copied as they are).
__global__ void __launch_bounds__(kThreads) rope_kv_write_seq_kernel(const uint16_t* __restrict__ qkv,
                                                                     const float* __restrict__ cos_t,
                                                                     const float* __restrict__ sin_t,
                                                                     uint16_t* __restrict__ q_out,
                                                                     uint16_t* __restrict__ kcache,
                                                                     uint16_t* __restrict__ vcache, int items, int S,
                                                                     int start, int H, int KVH, int hd, int ctx) {
  const int per_head = hd >> 4, heads = H + 2 * KVH;
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= items) return;
  const int c = i % per_head, head = (i / per_head) % heads, row = i / (per_head * heads);
  const int b = row / S, p = start + row % S;
  const int half = hd >> 1;
  const uint16_t* src = qkv + ((int64_t)row * heads + head) * hd + c * 8;
  const u32x4 v1 = *reinterpret_cast<const u32x4*>(src), v2 = *reinterpret_cast<const u32x4*>(src + half);
  uint16_t* dst;
  if (head < H) {
    dst = q_out + ((int64_t)row * H + head) * hd;
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
  load8f(cos_t + (int64_t)p * half + c * 8, cs);
  load8f(sin_t + (int64_t)p * half + c * 8, sn);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    o1[j] = x1[j] * cs[j] - x2[j] * sn[j];
    o2[j] = x1[j] * sn[j] + x2[j] * cs[j];
  }
  *reinterpret_cast<u32x4*>(dst) = pack8(o1);
  *reinterpret_cast<u32x4*>(dst + half) = pack8(o2);
}

// ---- causal attention over the cache, 128 query rows of one head per block ---------
// Block = (query tile, head, batch row); wave w owns query rows 32w .. 32w+31
// of the tile, one row per lane pair (lane l and l ^ 32 share row l & 31).
// Keys go by in tiles of 64, staged through registers into LDS (the next
// tile's loads are in flight during this tile's MFMAs):
//   K  [64][HD], its 16-B chunks XOR-swizzled by the key so that the 16 lanes
//      of a ds_read_b128 pass, which read one chunk column of 16 keys, hit 16
//      different bank groups;
//   Vᵀ [HD][64 + 4], written transposed (a thread turns 4 keys x 8 columns
//      into 8 stores of 4 keys), so that a PV operand is two 8-B reads.
// Scores come from the swapped product Sᵀ = mfma(K, Q): the accumulator has the
// query row on the lane and 16 keys in its registers, so the row maximum and
// sum are in-lane plus one exchange with lane ^ 32, and the registers, rounded
// to bf16 in pairs, are the B operand of Oᵀ = mfma(Vᵀ, Pᵀ) as they stand; Oᵀ
// again has the query row on the lane, so the online-softmax rescale is a
// per-lane scalar.  (Register 8t + j of lane half h is key 16t + 8(j>>2) + 4h
// + (j&3) of the 32: the Vᵀ operand is read in that same order.)
// A tile wholly above a wave's diagonal is skipped by that wave; tiles that
// cross it are masked per element with -inf before the maximum.  Cache rows
// >= start + S are not loaded (zeros are staged in their place, and masked).
// The register budget is held to two waves per SIMD (226 VGPRs at hd = 128, no
// scratch), so that two workgroups share a CU and one's softmax and barriers
// run under the other's MFMAs.
constexpr int kQTile = 128, kKTile = 64, kVStride = kKTile + 4;

template <int HD>
__global__ void __launch_bounds__(kThreads, 2) attn_prefill_kernel(const uint16_t* __restrict__ q,
                                                                const uint16_t* __restrict__ kcache,
                                                                const uint16_t* __restrict__ vcache,
                                                                uint16_t* __restrict__ out, int S, int start, int H,
                                                                int G, int KVH, int ctx, float scale_log2e) {
  constexpr int CH = HD / 8;                     // 16-B chunks per row
  constexpr int NK = kKTile * CH / kThreads;     // K chunks a thread stages: 4 or 2
  constexpr int SW = 16 / CH;                    // keys per 256 B of the K tile: 1 or 2
  constexpr int KS = HD / 16, DB = HD / 32;      // k-steps of QKᵀ, 32-column blocks of O
  __shared__ __attribute__((aligned(16))) uint16_t ks[kKTile * HD];
  __shared__ __attribute__((aligned(16))) uint16_t vt[HD * kVStride];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int h = blockIdx.y, b = blockIdx.z, kh = h / G;
  const int q0 = (gridDim.x - 1 - blockIdx.x) * kQTile;  // the long tiles first
  const int qw = q0 + wave * 32, qi = qw + r;
  const int n = start + S;                                 // keys 0..n-1 exist
  const int q_last = q0 + kQTile - 1 < S - 1 ? q0 + kQTile - 1 : S - 1;
  const int ntiles = (start + q_last) / kKTile + 1;
  const bool active = qw < S;
  const int wave_last = start + (qw + 31 < S - 1 ? qw + 31 : S - 1);  // the wave's last key
  const int lim = start + (qi < S - 1 ? qi : S - 1);                  // this row's last key

  // Q as the B operand of Sᵀ = K·Qᵀ: lane (r, hh) holds q[row r][16 s + 8 hh ..+8]; rows >= S are zeros.
  bf16x8_t qf[KS];
  {
    const u32x4* Q = reinterpret_cast<const u32x4*>(q + (((int64_t)b * S + (qi < S ? qi : 0)) * H + h) * HD);
#pragma unroll
    for (int s = 0; s < KS; ++s)
      qf[s] = __builtin_bit_cast(bf16x8_t, qi < S ? Q[2 * s + hh] : u32x4{0u, 0u, 0u, 0u});
  }
  const int64_t row0 = ((int64_t)b * KVH + kh) * ctx;
  const u32x4* Kg = reinterpret_cast<const u32x4*>(kcache) + row0 * CH;
  const u32x4* Vg = reinterpret_cast<const u32x4*>(vcache) + row0 * CH;

  // staging: K chunk e = tid + 256 i is (key e / CH, chunk e % CH); V unit tid is (4 keys tid / CH, chunk tid % CH)
  u32x4 kreg[NK], vreg[4];
  const bool vthread = tid < 16 * CH;
  const int vkg = tid / CH, vc = tid % CH;
  auto load_tile = [&](int kt) {
    const int k0 = kt * kKTile;
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int e = tid + kThreads * i, key = k0 + e / CH;
      kreg[i] = key < n ? Kg[(int64_t)key * CH + e % CH] : u32x4{0u, 0u, 0u, 0u};
    }
    if (vthread) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int key = k0 + 4 * vkg + i;
        vreg[i] = key < n ? Vg[(int64_t)key * CH + vc] : u32x4{0u, 0u, 0u, 0u};
      }
    }
  };
  auto stage_tile = [&]() {
#pragma unroll
    for (int i = 0; i < NK; ++i) {
      const int e = tid + kThreads * i, key = e / CH, c = e % CH;
      *reinterpret_cast<u32x4*>(ks + key * HD + ((c ^ ((key / SW) & (CH - 1))) << 3)) = kreg[i];
    }
    if (vthread) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const uint32_t a0 = vreg[0][w], a1 = vreg[1][w], a2 = vreg[2][w], a3 = vreg[3][w];
        uint16_t* dst = vt + (8 * vc + 2 * w) * kVStride + 4 * vkg;
        *reinterpret_cast<u32x2*>(dst) = u32x2{(a0 & 0xffffu) | (a1 << 16), (a2 & 0xffffu) | (a3 << 16)};
        *reinterpret_cast<u32x2*>(dst + kVStride) =
            u32x2{(a0 >> 16) | (a1 & 0xffff0000u), (a2 >> 16) | (a3 & 0xffff0000u)};
      }
    }
  };

  f32x16_t oacc[DB];
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int i = 0; i < 16; ++i) oacc[d][i] = 0.0f;
  float m = -INFINITY, l = 0.0f;  // l: this lane's half of the keys

  load_tile(0);
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();  // every wave is done reading the previous tile
    stage_tile();
    __syncthreads();
    if (kt + 1 < ntiles) load_tile(kt + 1);
    const int k0 = kt * kKTile;
    if (!active || k0 > wave_last) continue;  // wave-uniform

    f32x16_t sacc[2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb) {
#pragma unroll
      for (int i = 0; i < 16; ++i) sacc[kb][i] = 0.0f;
      const int key = kb * 32 + r;
      const uint16_t* krow = ks + key * HD;
      const int sw = (key / SW) & (CH - 1);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const bf16x8_t a =
            __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4*>(krow + (((2 * s + hh) ^ sw) << 3)));
        sacc[kb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, qf[s], sacc[kb], 0, 0, 0);
      }
    }
    // scale (fp32), mask, row maximum
    const bool masked = k0 + kKTile - 1 > start + qw;  // wave-uniform: some row of the wave ends inside the tile
    float mx = m;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int key = k0 + kb * 32 + (i & 3) + 8 * (i >> 2) + 4 * hh;
        float v = sacc[kb][i] * scale_log2e;
        if (masked && key > lim) v = -INFINITY;
        sacc[kb][i] = v;
        mx = fmaxf(mx, v);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float alpha = exp2_diff(m, mx);
    m = mx;
    float ps = 0.0f;
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float p = exp2_diff(sacc[kb][i], mx);
        sacc[kb][i] = p;
        ps += p;
      }
    l = l * alpha + ps;
#pragma unroll
    for (int d = 0; d < DB; ++d)
#pragma unroll
      for (int i = 0; i < 16; ++i) oacc[d][i] *= alpha;
    // P rounded to bf16: registers 8t .. 8t+7 of block kb are the B fragment of k-step (kb, t)
    bf16x8_t pf[2][2];
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int t = 0; t < 2; ++t)
        pf[kb][t] = __builtin_bit_cast(
            bf16x8_t, u32x4{pack2(sacc[kb][8 * t], sacc[kb][8 * t + 1]), pack2(sacc[kb][8 * t + 2], sacc[kb][8 * t + 3]),
                            pack2(sacc[kb][8 * t + 4], sacc[kb][8 * t + 5]),
                            pack2(sacc[kb][8 * t + 6], sacc[kb][8 * t + 7])});
#pragma unroll
    for (int d = 0; d < DB; ++d) {
      const uint16_t* vrow = vt + (32 * d + r) * kVStride + 4 * hh;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const u32x2 lo = *reinterpret_cast<const u32x2*>(vrow + kb * 32 + 16 * t);
          const u32x2 hi = *reinterpret_cast<const u32x2*>(vrow + kb * 32 + 16 * t + 8);
          const bf16x8_t a = __builtin_bit_cast(bf16x8_t, u32x4{lo.x, lo.y, hi.x, hi.y});
          oacc[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, pf[kb][t], oacc[d], 0, 0, 0);
        }
    }
  }

  if (!active) return;
  l += __shfl_xor(l, 32, 64);
  if (qi >= S) return;  // a tail tile's rows beyond the prompt are never stored
  const float inv = 1.0f / l;  // l >= 1: key 0 is visible to every row, and the maximum's own term is 1
  uint16_t* orow = out + (((int64_t)b * S + qi) * H + h) * HD + 4 * hh;
#pragma unroll
  for (int d = 0; d < DB; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<u32x2*>(orow + 32 * d + 8 * g) =
          u32x2{pack2(oacc[d][4 * g] * inv, oacc[d][4 * g + 1] * inv),
                pack2(oacc[d][4 * g + 2] * inv, oacc[d][4 * g + 3] * inv)};
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

// The kernels index tokens, keys and grid blocks with int and form every
// element offset in int64: a shape passes when B and H fit a grid dimension,
// ctx leaves room for a key tile past it, and the RoPE kernel's thread count
// fits an int.
VGPU_API int vgpu_prefill_supported(int B, int S, int start, int H, int KVH, int hd, int ctx) {
  if (B < 1 || S < 1 || start < 0 || ctx < 1 || (int64_t)start + S > ctx) return 0;
  if (hd != 64 && hd != 128) return 0;
  if (H < 1 || KVH < 1 || H % KVH || H / KVH > 8) return 0;
  if (B > 65535 || H > 65535 || ctx > (1 << 30)) return 0;
  if ((int64_t)B * S * (H + 2 * KVH) * (hd / 16) > INT32_MAX - kThreads) return 0;
  return 1;
}

// qkv [B·S][(H+2·KVH)·hd] bf16, row b·S + s; cos, sin [max_seq][hd/2] fp32, row start + s.
// q_out [B][S][H][hd]; caches [B][KVH][ctx][hd], rows start .. start+S-1 written (k rotated, v as it is).
VGPU_API int vgpu_rope_kv_write_seq(const void* qkv, const void* cos_t, const void* sin_t, void* q_out, void* kcache,
                                    void* vcache, int B, int S, int start, int H, int KVH, int hd, int ctx,
                                    int max_seq, hipStream_t s) {
  if (!vgpu_prefill_supported(B, S, start, H, KVH, hd, ctx) || (int64_t)start + S > max_seq) return -1;
  if (!qkv || !cos_t || !sin_t || !q_out || !kcache || !vcache) return -1;
  if (!al16(qkv) || !al16(cos_t) || !al16(sin_t) || !al16(q_out) || !al16(kcache) || !al16(vcache)) return -1;
  const int items = B * S * (H + 2 * KVH) * (hd / 16);
  hipLaunchKernelGGL(rope_kv_write_seq_kernel, dim3((items + kThreads - 1) / kThreads), dim3(kThreads), 0, s,
                     (const uint16_t*)qkv, (const float*)cos_t, (const float*)sin_t, (uint16_t*)q_out,
                     (uint16_t*)kcache, (uint16_t*)vcache, items, S, start, H, KVH, hd, ctx);
  return (int)hipGetLastError();
}

// out [B][S][H·hd] = causal attention of q [B][S][H][hd] over cache rows 0 .. start+i
// (query head h reads kv head h / (H/KVH)); scale > 0 is applied to the fp32 scores.
VGPU_API int vgpu_attn_prefill(const void* q, const void* kcache, const void* vcache, void* out, int B, int S,
                               int start, int H, int KVH, int hd, int ctx, float scale, hipStream_t s) {
  if (!vgpu_prefill_supported(B, S, start, H, KVH, hd, ctx) || !(scale > 0.0f) || !(scale < INFINITY)) return -1;
  if (!q || !kcache || !vcache || !out || !al16(q) || !al16(kcache) || !al16(vcache) || !al16(out)) return -1;
  const dim3 grid((S + kQTile - 1) / kQTile, H, B);
  const float sl2 = scale * 1.44269504088896341f;
  if (hd == 128)
    hipLaunchKernelGGL(attn_prefill_kernel<128>, grid, dim3(kThreads), 0, s, (const uint16_t*)q,
                       (const uint16_t*)kcache, (const uint16_t*)vcache, (uint16_t*)out, S, start, H, H / KVH, KVH,
                       ctx, sl2);
  else
    hipLaunchKernelGGL(attn_prefill_kernel<64>, grid, dim3(kThreads), 0, s, (const uint16_t*)q,
                       (const uint16_t*)kcache, (const uint16_t*)vcache, (uint16_t*)out, S, start, H, H / KVH, KVH,
                       ctx, sl2);
  return (int)hipGetLastError();
}
