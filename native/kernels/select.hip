// Token selection on the device, after the head GEMV of a Llama decode step:
// greedy (argmax) and temperature / top-k / top-p sampling over bf16 logits
// [B][V], fused with the bookkeeping that closes the decode loop (the chosen
// token into the buffer the next embedding reads, `pos` and `step` advanced).
//
// Ordering of logits (everything below selects by it):
//   - logits compare as values, with +0 == -0;
//   - NaN ranks below -inf;
//   - ties go to the lowest index;
//   - hence a row of all NaN selects index 0.
// It is realised as a 16-bit order key of the bf16 bit pattern (larger key =
// earlier in the ordering): NaN -> 0, -0 -> the key of +0, sign clear ->
// bits | 0x8000, sign set -> ~bits.  -inf gets 0x007f, +inf 0xff80.
//
//   greedy   the first element of the ordering.  A partial launch on a grid of
//            (chunk, row) writes one (key, index) per chunk into the workspace;
//            a combine launch of one workgroup merges them for all rows.
//   sample   candidates c_0..c_{k-1}: the first k elements of the ordering
//            (k = top_k <= 64).  l[c_0] not finite: the token is c_0.  Else
//            w_j = exp((l[c_j] - l[c_0]) / T) in fp32 (a NaN candidate weighs
//            0), W_k = sum of all k; nucleus = smallest m >= 1 with
//            sum_{j<m} w_j >= top_p * W_k; token = c_j for the smallest j < m
//            with sum_{i<=j} w_i > u * W_m, or c_{m-1} when rounding leaves
//            none.  Sums run in candidate order.  top_p acts inside the top-k
//            set; there is no nucleus over the whole vocabulary.
//            The partial launch finds each chunk's own first k by an exact
//            two-level radix select on the key (8 bits a level, histograms in
//            LDS), takes everything above the cut plus the lowest-index
//            elements equal to it, and sorts them; the final launch, one
//            workgroup, does the same over the chunks' lists (the first k of
//            the row are among the first k of each chunk), from a copy of
//            the lists in LDS while they fit (up to 64 chunks), and draws.
//   advance  in the last launch of either, with s = *step: s outside [0, T)
//            writes nothing at all.  Else per row t = the selected token, or
//            eos when eos >= 0, s > 0 and out[b][s-1] == eos (sticky);
//            out[b][s] = t, next_tok[b] = t; after a barrier one thread stores
//            *step = s + 1 and *pos = *pos + 1.
//
// The working set is 256 KB a row at V = 128 256, just written by the head
// GEMV: latency-bound, so few short dispatches, one 16-B load per thread.
// Grids depend on shapes only and `step` / `pos` are read on the device, so
// the launches capture into a graph and replay at any step.  No global
// atomics, no hand-off between workgroups inside a launch: the same inputs
// give the same bits.  The LDS counters are integer counts, which do not
// depend on the order of their increments; every list position comes from a
// scan in thread order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16.h"

namespace {

constexpr int kWaves = kThreads / 64;
constexpr int kChunk = kThreads * 8;  // logits per block of a partial launch: one 16-B load per thread
constexpr int kMaxTopK = 64;
constexpr int kStage = 4096;  // candidates a row's final select holds in LDS: 64 chunks of 64 (V <= 131 072)

__device__ __forceinline__ uint32_t order_key(uint32_t bits) {
  bits &= 0xffffu;
  if ((bits & 0x7fffu) > 0x7f80u) return 0u;  // NaN: last
  if (bits == 0x8000u) bits = 0u;             // -0 is +0
  return (bits & 0x8000u) ? (~bits & 0xffffu) : (bits | 0x8000u);
}
// The logit a key stands for (never called on the NaN key).
__device__ __forceinline__ float key_value(uint32_t key) {
  const uint32_t bits = (key & 0x8000u) ? (key & 0x7fffu) : (~key & 0xffffu);
  return __uint_as_float(bits << 16);
}
__device__ __forceinline__ uint64_t ranked(uint32_t key, uint32_t idx) {
  return ((uint64_t)key << 32) | (uint32_t)~idx;  // max = largest key, then lowest index
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}

// ---- advance: the tail of the last launch (one workgroup; tok in LDS, filled before the call) ----
__device__ __forceinline__ void advance(const int* tok, int B, int64_t s, int64_t* __restrict__ step,
                                        int64_t* __restrict__ pos, int64_t* __restrict__ next_tok,
                                        int64_t* __restrict__ out, int T, int eos) {
  __syncthreads();
  if ((int)threadIdx.x < B) {
    const int b = threadIdx.x;
    int64_t t = tok[b];
    if (eos >= 0 && s > 0 && out[(int64_t)b * T + s - 1] == (int64_t)eos) t = eos;
    out[(int64_t)b * T + s] = t;
    next_tok[b] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    *step = s + 1;
    *pos = *pos + 1;
  }
}

// ---- greedy ----------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) greedy_partial_kernel(const uint16_t* __restrict__ logits,
                                                                  uint2* __restrict__ ws, int V, int chunks) {
  __shared__ uint64_t part[kWaves];
  const int c = blockIdx.x, b = blockIdx.y;
  const int e0 = c * kChunk + (int)threadIdx.x * 8;
  uint64_t best = 0;  // no element: below ranked() of any real one (its low word, ~index, is never 0)
  if (e0 < V) {       // V % 8 == 0: the 8 are all inside
    const u32x4 v = *reinterpret_cast<const u32x4*>(logits + (int64_t)b * V + e0);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint64_t r = ranked(order_key(w[j >> 1] >> ((j & 1) * 16)), (uint32_t)(e0 + j));
      best = r > best ? r : best;
    }
  }
  best = wave_max(best);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kWaves; ++w) best = part[w] > best ? part[w] : best;
    ws[(int64_t)b * chunks + c] = uint2{(uint32_t)(best >> 32), ~(uint32_t)best};
  }
}

// One workgroup: wave w merges rows w, w + 4 over their chunks (in chunk order per lane), then advance.
__global__ void __launch_bounds__(kThreads) greedy_combine_kernel(const uint2* __restrict__ ws, int B, int chunks,
                                                                  int64_t* __restrict__ step,
                                                                  int64_t* __restrict__ pos,
                                                                  int64_t* __restrict__ next_tok,
                                                                  int64_t* __restrict__ out, int T, int eos) {
  __shared__ int tok[8];
  const int64_t s = *step;
  if (s < 0 || s >= T) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += kWaves) {
    uint64_t best = 0;
    for (int c = lane; c < chunks; c += 64) {
      const uint2 p = ws[(int64_t)b * chunks + c];
      const uint64_t r = ranked(p.x, p.y);
      best = r > best ? r : best;
    }
    best = wave_max(best);
    if (lane == 0) tok[b] = (int)~(uint32_t)best;
  }
  advance(tok, B, s, step, pos, next_tok, out, T, eos);
}

// ---- the first k of n items, held by a workgroup ---------------------------------------
struct TopK {
  int hist[256];
  int wsum[kWaves];
  int pick[2];
  uint32_t ckey[kMaxTopK], cidx[kMaxTopK];  // as gathered
  uint32_t skey[kMaxTopK], sidx[kMaxTopK];  // in order
};

// Inclusive scan of one int per thread, in thread order.
__device__ __forceinline__ int block_scan(TopK& sh, int v) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(v, o, 64);
    if (lane >= o) v += up;
  }
  __syncthreads();  // the previous scan's wsum has been read
  if (lane == 63) sh.wsum[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += sh.wsum[w];
  return v;
}

// From the histogram: the highest bin whose count, with all bins above it,
// reaches k -> pick[0]; how many of that bin are wanted -> pick[1].  Needs
// 1 <= k <= the histogram's total.
__device__ __forceinline__ void find_bin(TopK& sh, int k) {
  const int bin = 255 - (int)threadIdx.x;  // thread order = from the top bin down
  const int h = sh.hist[bin];
  const int incl = block_scan(sh, h);
  if (incl >= k && incl - h < k) {
    sh.pick[0] = bin;
    sh.pick[1] = k - (incl - h);
  }
  __syncthreads();
}

// The first min(k, n) of items 0..n-1 in the ordering (key descending, then
// item order, which must be index order among equal keys) into sh.skey /
// sh.sidx; returns their number.  Thread t holds items [t per, (t + 1) per);
// per * kThreads >= n.  key_at(i) is the 16-bit order key, idx_at(i) the index.
template <class KeyAt, class IdxAt>
__device__ __forceinline__ int block_topk(TopK& sh, int n, int per, int k, KeyAt key_at, IdxAt idx_at) {
  const int t = threadIdx.x;
  const int i0 = t * per < n ? t * per : n, i1 = i0 + per < n ? i0 + per : n;
  if (k > n) k = n;
  sh.hist[t] = 0;
  __syncthreads();
  for (int i = i0; i < i1; ++i) atomicAdd(&sh.hist[key_at(i) >> 8], 1);
  __syncthreads();
  find_bin(sh, k);
  const uint32_t hi = sh.pick[0];
  const int k2 = sh.pick[1];
  sh.hist[t] = 0;
  __syncthreads();
  for (int i = i0; i < i1; ++i) {
    const uint32_t key = key_at(i);
    if ((key >> 8) == hi) atomicAdd(&sh.hist[key & 255u], 1);
  }
  __syncthreads();
  find_bin(sh, k2);
  const uint32_t cut = (hi << 8) | (uint32_t)sh.pick[0];
  const int need = sh.pick[1], above = k - need;  // `above` items beat the cut; `need` of those equal to it go in

  int na = 0, ne = 0;
  for (int i = i0; i < i1; ++i) {
    const uint32_t key = key_at(i);
    na += key > cut;
    ne += key == cut;
  }
  const int mine = (ne << 8) | na;  // fewer than 64 above in all, so the low byte never carries
  const int excl = block_scan(sh, mine) - mine;
  int ea = excl & 255, ee = excl >> 8;
  for (int i = i0; i < i1; ++i) {
    const uint32_t key = key_at(i);
    int slot = -1;
    if (key > cut) {
      slot = ea++;
    } else if (key == cut) {
      if (ee < need) slot = above + ee;
      ++ee;
    }
    if (slot >= 0) {
      sh.ckey[slot] = key;
      sh.cidx[slot] = idx_at(i);
    }
  }
  __syncthreads();
  if (t < k) {  // rank sort: at most 64 entries, all (key, index) pairs distinct
    const uint32_t key = sh.ckey[t], idx = sh.cidx[t];
    int r = 0;
    for (int j = 0; j < k; ++j) r += sh.ckey[j] > key || (sh.ckey[j] == key && sh.cidx[j] < idx);
    sh.skey[r] = key;
    sh.sidx[r] = idx;
  }
  __syncthreads();
  return k;
}

// ---- sampling --------------------------------------------------------------------------
// Block (chunk, row): the chunk's first min(k, len) elements, in order, into
// ws[(row chunks + chunk) kMaxTopK + 0..].
__global__ void __launch_bounds__(kThreads) sample_partial_kernel(const uint16_t* __restrict__ logits,
                                                                  uint2* __restrict__ ws, int V, int chunks, int k) {
  __shared__ TopK sh;
  __shared__ __attribute__((aligned(16))) uint16_t keys[kChunk];
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int base = c * kChunk;
  const int len = V - base < kChunk ? V - base : kChunk;
  if (t * 8 < len) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(logits + (int64_t)b * V + base + t * 8);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = order_key(w[j]) | (order_key(w[j] >> 16) << 16);
    *reinterpret_cast<u32x4*>(keys + t * 8) = u32x4{o[0], o[1], o[2], o[3]};
  }
  __syncthreads();
  const int m = block_topk(sh, len, 8, k, [&](int i) { return (uint32_t)keys[i]; },
                           [&](int i) { return (uint32_t)(base + i); });
  if (t < m) ws[((int64_t)b * chunks + c) * kMaxTopK + t] = uint2{sh.skey[t], sh.sidx[t]};
}

// One workgroup, the rows one after another: the first k of the chunks' lists
// (chunk order, each list in order: index order among equal keys), the draw, advance.
__global__ void __launch_bounds__(kThreads) sample_final_kernel(const uint2* __restrict__ ws, int B, int V,
                                                                int chunks, int k, float temperature, float top_p,
                                                                const float* __restrict__ u,
                                                                int64_t* __restrict__ step, int64_t* __restrict__ pos,
                                                                int64_t* __restrict__ next_tok,
                                                                int64_t* __restrict__ out, int T, int eos) {
  __shared__ TopK sh;
  __shared__ uint2 items[kStage];
  __shared__ float wgt[kMaxTopK];
  __shared__ int tok[8];
  const int64_t s = *step;
  if (s < 0 || s >= T) return;
  const int t = threadIdx.x;
  const int last_len = V - (chunks - 1) * kChunk;
  const int full = (chunks - 1) * k;  // every chunk but the last is whole and lists k (k <= 64 < kChunk)
  const int n = full + (k < last_len ? k : last_len);
  const int per = (n + kThreads - 1) / kThreads;
  for (int b = 0; b < B; ++b) {
    const uint2* row = ws + (int64_t)b * chunks * kMaxTopK;
    auto at = [&](int i) -> const uint2& {
      const int c = i < full ? i / k : chunks - 1, slot = i < full ? i % k : i - full;
      return row[(int64_t)c * kMaxTopK + slot];
    };
    int m;
    if (n <= kStage) {  // the usual case: one coalesced pass brings the lists into LDS, the select reads them there
      __syncthreads();  // the previous row is done with `items`
      for (int i = t; i < n; i += kThreads) items[i] = at(i);
      __syncthreads();
      m = block_topk(sh, n, per, k, [&](int i) { return items[i].x; }, [&](int i) { return items[i].y; });
    } else {
      m = block_topk(sh, n, per, k, [&](int i) { return at(i).x; }, [&](int i) { return at(i).y; });
    }
    const uint32_t key0 = sh.skey[0];
    const float l0 = key0 ? key_value(key0) : NAN;
    const bool finite = key0 != 0u && fabsf(l0) != INFINITY;
    if (t < m) {
      const uint32_t key = sh.skey[t];
      wgt[t] = (finite && key != 0u) ? expf((key_value(key) - l0) / temperature) : 0.0f;
    }
    __syncthreads();
    if (t == 0) {
      int j = 0;
      if (finite) {
        float Wk = 0.0f;
        for (int i = 0; i < m; ++i) Wk += wgt[i];
        const float want = top_p * Wk;
        float Wm = 0.0f;
        int nuc = 0;
        do Wm += wgt[nuc++]; while (nuc < m && !(Wm >= want));
        const float draw = u[s * B + b] * Wm;
        float acc = 0.0f;
        j = nuc - 1;
        for (int i = 0; i < nuc; ++i) {
          acc += wgt[i];
          if (acc > draw) {
            j = i;
            break;
          }
        }
      }
      tok[b] = (int)sh.sidx[j];
    }
    __syncthreads();
  }
  advance(tok, B, s, step, pos, next_tok, out, T, eos);
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool al8(const void* p) { return ((uintptr_t)p & 7u) == 0; }
inline bool batch_ok(int B) { return B == 1 || B == 2 || B == 3 || B == 4 || B == 8; }
inline int chunks_of(int V) { return (V + kChunk - 1) / kChunk; }

}  // namespace

// Logits [B][V] bf16: B in 1-4 or 8, V a multiple of 8 (below 2^30), 1 <= top_k <= 64 (greedy: pass 1).
VGPU_API int vgpu_select_supported(int B, int V, int top_k) {
  return batch_ok(B) && V >= 8 && V % 8 == 0 && V <= (1 << 30) && top_k >= 1 && top_k <= kMaxTopK;
}

// Logits per block of the partial launches: a function of V alone (the grid is frozen in a captured graph).
VGPU_API int vgpu_select_chunk(int V) { return V >= 8 && V % 8 == 0 ? kChunk : -1; }

// Workspace (bytes) of either selection: a (key, index) pair per (row, chunk, candidate).
VGPU_API int64_t vgpu_select_workspace(int B, int V) {
  if (B < 1 || V < 8 || V % 8) return -1;
  return (int64_t)B * chunks_of(V) * kMaxTopK * (int64_t)sizeof(uint2);
}

static int select_args_ok(const void* logits, const void* ws, int64_t ws_bytes, int B, int V, int top_k,
                          const void* step, const void* pos, const void* next_tok, const void* out, int T) {
  if (!vgpu_select_supported(B, V, top_k) || T < 1) return 0;
  if (!logits || !ws || !step || !pos || !next_tok || !out) return 0;
  if (!al16(logits) || !al8(ws) || !al8(step) || !al8(pos) || !al8(next_tok) || !al8(out)) return 0;
  return ws_bytes >= vgpu_select_workspace(B, V);
}

// next_tok [B][1], out [B][T] (column *step), step [1], pos [1]: device int64.  eos: -1 for none.
VGPU_API int vgpu_select_greedy(const void* logits, void* ws, int64_t ws_bytes, int B, int V, void* step, void* pos,
                                void* next_tok, void* out, int T, int eos, hipStream_t s) {
  if (!select_args_ok(logits, ws, ws_bytes, B, V, 1, step, pos, next_tok, out, T)) return -1;
  const int chunks = chunks_of(V);
  hipLaunchKernelGGL(greedy_partial_kernel, dim3(chunks, B), dim3(kThreads), 0, s, (const uint16_t*)logits,
                     (uint2*)ws, V, chunks);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(greedy_combine_kernel, dim3(1), dim3(kThreads), 0, s, (const uint2*)ws, B, chunks,
                     (int64_t*)step, (int64_t*)pos, (int64_t*)next_tok, (int64_t*)out, T, eos);
  return (int)hipGetLastError();
}

// u [T][B] fp32 in [0, 1), row *step read; temperature > 0, 0 < top_p <= 1.
VGPU_API int vgpu_select_sample(const void* logits, void* ws, int64_t ws_bytes, int B, int V, float temperature,
                                int top_k, float top_p, const void* u, void* step, void* pos, void* next_tok,
                                void* out, int T, int eos, hipStream_t s) {
  if (!select_args_ok(logits, ws, ws_bytes, B, V, top_k, step, pos, next_tok, out, T)) return -1;
  if (!(temperature > 0.0f) || !(top_p > 0.0f) || !(top_p <= 1.0f) || !u || ((uintptr_t)u & 3u)) return -1;
  const int chunks = chunks_of(V);
  hipLaunchKernelGGL(sample_partial_kernel, dim3(chunks, B), dim3(kThreads), 0, s, (const uint16_t*)logits,
                     (uint2*)ws, V, chunks, top_k);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sample_final_kernel, dim3(1), dim3(kThreads), 0, s, (const uint2*)ws, B, V, chunks, top_k,
                     temperature, top_p, (const float*)u, (int64_t*)step, (int64_t*)pos, (int64_t*)next_tok,
                     (int64_t*)out, T, eos);
  return (int)hipGetLastError();
}
