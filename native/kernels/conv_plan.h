// Kernel selection for conv_gemm.hip: which kernel family, tile and split count
// a convolution runs with, as a pure function of the request and the process's
// knobs.  Plain C++17, no HIP: tests/test_conv_plan_cpu.py compiles it with g++.
// Every batch slice is planned before the first launch, so whatever makes a
// conv unsupported is decided here.  Req is conv_gemm.hip's ConvArgs as an entry
// point fills it (or any struct with its N H W C Cout stride pad act res_stride
// and, for "is it there", pscale res bias stats bnx qscale gmask ws).
#pragma once

#include <stdint.h>

namespace convplan {

// What the process runs on and what its A/B setters and environment force.
struct ConvKnobs {
  int cus;           // conv_cus(): CUs this process can occupy
  int forced_bm;     // vgpu_conv_set_tile_m: 0 = heuristic
  int forced_big;    // vgpu_conv_set_big: -1 = env_big, 0 = off, 1 = whenever eligible, 2 = heuristic
  int forced_halo;   // vgpu_conv_set_halo: -1 = env_halo, 0 = off, 1 = on, 2 / 3 = on with BM 256 / 128
  int forced_split;  // vgpu_conv_set_splitk: -1 heuristic, 0 off, n > 1 that many splits when eligible
  int env_big;       // VGPU_CONV_BIG in forced_big's terms: '1' 1, '0' 0, otherwise / unset 2
  bool env_halo, env_1x1_big;  // VGPU_CONV_HALO (halo_enabled()), VGPU_CONV_1X1_BIG (conv_1x1_big())
};

enum class Family { unsupported, gemm, pro, glds, big, halo };

// One batch slice's launch: nM x nN workgroups of `threads` of
//   gemm  conv_gemm_kernel<KS, BM, BN, RES> (persistent: the launcher caps the grid)
//   pro   conv_pro_kernel<KS, BM, BN, RES>
//   glds  conv_glds_kernel<KS, BM, BN, RES, CSM, ST, splits > 1, POST>; split: grid y =
//         splits, POST moves to the splitk_reduce_kernel<POST> that follows
//   big   conv_big_kernel<RES, 4>
//   halo  conv_halo_kernel<BM, BN, BM * 3 / 2, ST>
struct ConvPlan {
  Family family = Family::unsupported;
  int nb = 0;  // images in the slice; the full slices of a batch have the same
  int KS = 0, BM = 0, BN = 0, CSM = 0, ST = 0, threads = 256;
  bool RES = false, POST = false;
  int splits = 1, kper = 0, nM = 0, nN = 0, nmajor = 0;
  bool ok() const { return family != Family::unsupported; }
  bool past_split() const { return BM != 0 && splits <= 1; }  // got to the unsplit kernels' rules
};

inline int out_size(int in, int ks, int stride, int pad) { return (in + 2 * pad - ks) / stride + 1; }

// C % 64 == 0 with 1x1 / 3x3 filters, or the narrow stem form (C = 16, 4x4,
// stride 1, no prologue: a 7x7/s2 conv on a space-to-depth input).
inline bool conv_narrow(int C, int KS, int stride, bool pro) { return C == 16 && KS == 4 && stride == 1 && !pro; }

// Split-K for convs whose output tiles cannot fill the CUs this process owns:
// the 28² / 14² layers of VGG-16 at batch 2 are 16-100 workgroups of 64x128 on
// 256 CUs (36-41 us each, ~8 % of MFMA peak; profiles/r5/train).  The K steps
// are cut into `splits` ranges so ~2 workgroups per CU run, each writing an
// fp32 partial tile, and splitk_reduce_kernel applies the epilogue.  Returns
// the split count (1 = no split) and the K steps per split.
inline int splitk_plan(int64_t M, int C, int Cout, int KS, bool pro, bool narrow, const ConvKnobs& k, int& kper) {
  const int ktiles = KS * KS * C / 64;
  kper = ktiles;
  if (pro || narrow || C % 64 || (KS != 1 && KS != 3) || k.forced_split == 0) return 1;
  // a kernel forced by an A/B or test setter runs as asked unless splits are forced too
  if (k.forced_split < 0 && (k.forced_halo >= 0 || k.forced_big == 1 || k.forced_bm != 0)) return 1;
  const int bn = Cout % 128 == 0 ? 128 : 64;
  const int64_t tiles = ((M + 63) / 64) * (Cout / bn);
  // Measured (profiles/r5/train/vgg_small_ab.log, graph replay): 100 and 28
  // tiles gain 1.2-1.8x; 196 tiles (56² at b=2) lose 17 % -- split below half the CUs.
  int64_t sp = k.forced_split > 1 ? k.forced_split : (2 * tiles >= k.cus ? 1 : 2 * (int64_t)k.cus / tiles);
  if (sp > ktiles / 4) sp = ktiles / 4;
  if (sp < 2) return 1;
  kper = (int)((ktiles + sp - 1) / sp);
  return (ktiles + kper - 1) / kper;
}

// Workspace (bytes) a split-K launch of this shape wants; 0 when the conv runs unsplit.
inline int64_t conv_workspace(int N, int H, int W, int C, int Cout, int KS, int stride, int pad, bool pro,
                              const ConvKnobs& k) {
  if (N < 1 || stride < 1 || pad < 0 || KS < 1) return 0;
  const int64_t OH = out_size(H, KS, stride, pad), OW = out_size(W, KS, stride, pad);
  if (OH < 1 || OW < 1) return 0;
  const int64_t M = (int64_t)N * OH * OW;
  int kper;
  const int sp = splitk_plan(M, C, Cout, KS, pro, conv_narrow(C, KS, stride, pro), k, kper);
  return sp > 1 ? (int64_t)sp * M * Cout * 4 : 0;
}

// Halo pixels a BM-pixel tile of a W-wide image can need: rows spanned + 2.
inline int halo_pixels(int bm, int w) { return ((bm - 1) / w + 4) * w; }

// The plan of the batch's full slices, or with `last` that of its last slice,
// which may be shorter than the others and choose a different tile.
template <class Req>
ConvPlan conv_plan(const Req& a, int KS, int64_t ws_bytes, const ConvKnobs& k, bool last) {
  ConvPlan p;
  const int C = a.C, Cout = a.Cout;
  const bool pro = a.pscale != nullptr, has_res = a.res != nullptr, stats = a.stats != nullptr;
  const bool post = a.qscale != nullptr, narrow = conv_narrow(C, KS, a.stride, pro);
  if (a.act < 0 || a.act > 2 || (!narrow && (C % 64 || (KS != 1 && KS != 3)))) return p;
  if (Cout % 64 || a.stride < 1 || a.pad < 0 || a.N < 1) return p;
  const int OH = out_size(a.H, KS, a.stride, a.pad), OW = out_size(a.W, KS, a.stride, a.pad);
  if (OH < 1 || OW < 1 || (stats && (narrow || pro))) return p;
  if (narrow && has_res) return p;  // the narrow kernels have no residual form: refuse, never drop it
  if (a.res_stride == 2 && (int64_t)a.N * ((OH + 1) / 2) * ((OW + 1) / 2) * Cout * 2 >= ((int64_t)1 << 31)) return p;
  // Post epilogue: the 1x1 + residual LDS-DMA kernels (and their split-K reduce) only.
  if (post && (KS != 1 || pro || !has_res || stats || a.gmask || a.act != 0 || a.bias)) return p;
  // Buffer offsets are 32-bit: the batch runs in slices whose activations stay < 2 GiB.
  const int64_t xi = (int64_t)a.H * a.W * C * 2, yi = (int64_t)OH * OW * Cout * 2;
  const int64_t per = (((int64_t)1 << 31) - 1) / (xi > yi ? xi : yi);
  if (per < 1 || (per < a.N && (stats || post))) return p;  // statistics: one slice (group rows are global); so is post
  const int nfull = (int)(per < a.N ? per : a.N);
  p.nb = last && a.N % nfull ? a.N % nfull : nfull;
  const int M = p.nb * OH * OW;
  const int ktiles = KS * KS * C / 64;
  const int bn = (Cout % 128 == 0) ? 128 : 64;
  // Small-M layers use 64-row tiles so the grid still fills the CUs this
  // process owns: 128-row tiles fetch fewer bytes per FLOP, but below ~1.5
  // workgroups per CU the kernel is latency-bound (profiles/conv_cus_r1.md:
  // exclusive 256 CUs and 50 % pods of 128 CUs agree with this threshold).
  const int64_t tiles128 = (int64_t)((M + 127) / 128) * (Cout / bn);
  bool small = tiles128 < (int64_t)k.cus * 3 / 2;
  // Non-prologue 1x1 convs (conv3 + residual) are DMA/HBM-bound: 64-row tiles
  // (48 KB LDS → 3 blocks per CU) beat 128-row tiles on every ResNet-50 shape
  // (profiles/conv_tiles_r1.md).  Without a residual, from K = 256 and 128
  // outputs up -- a projection block's shortcut and conv1 on a pre-activated
  // input -- 128-row tiles measured 2-7 % ahead on all six such flagship
  // shapes (profiles/r7/preact), so those keep the grid-fill rule above;
  // K = 64 (block 0) stays on 64-row tiles (tie / 6 % behind).
  const bool rows128_ok = !has_res && !stats && C >= 256 && Cout >= 128;
  if (!pro && KS == 1 && !rows128_ok) small = !k.env_1x1_big;
  if (k.forced_bm == 64) small = true;
  if (k.forced_bm == 128) small = false;
  int kper;
  const int splits = (a.ws && !stats && per >= a.N) ? splitk_plan(M, C, Cout, KS, pro, narrow, k, kper) : 1;
  if (a.gmask && splits <= 1) return p;  // the masked form exists only as a split-K reduce
  if (splits > 1 && ws_bytes < (int64_t)splits * M * Cout * 4) return p;
  p.KS = KS;
  p.BM = small || splits > 1 ? 64 : 128;
  p.BN = bn;
  p.RES = has_res && splits <= 1;  // split: the reduce adds the residual
  p.ST = stats ? (a.bnx ? 2 : 1) : 0;
  p.POST = post;
  p.splits = splits;
  p.kper = splits > 1 ? kper : ktiles;
  Family f = pro ? Family::gemm : Family::glds;
  // 256x256 tiles: 1x1 / stride 1 / no prologue, Cout % 256 == 0, deep K
  // (≥ 1024: below it these layers are HBM-bound and the 64-row tiles at 3
  // blocks per CU win — the ResNet-50 flagship measured 1 % slower with the
  // big tile on its K = 128-512 conv3 layers), and enough tiles to give every
  // CU this process owns at least one.
  const int big_mode = k.forced_big < 0 ? k.env_big : k.forced_big;
  const bool big_ok = !narrow && !pro && KS == 1 && a.stride == 1 && a.pad == 0 && Cout % 256 == 0 && C >= 128;
  const int64_t tiles256 = (int64_t)((M + 255) / 256) * (Cout / 256);
  const bool big = !stats && big_ok && (big_mode == 1 || (big_mode == 2 && C >= 1024 && tiles256 >= (int64_t)k.cus));
  // 3x3 / stride 1 without prologue or residual: the halo-tile kernel, when Cout % 128 == 0
  // and a tile's halo fits the LDS image (BM * 3 / 2 pixels, the last one a zero row).
  const bool halo = (k.forced_halo < 0 ? k.env_halo : k.forced_halo > 0) && !narrow && !pro && !has_res && KS == 3 &&
                    a.stride == 1 && a.pad == 1 && Cout % 128 == 0;
  const int64_t htiles256 = (int64_t)((M + 255) / 256) * (Cout / 128);
  const bool hbig = k.forced_halo == 2 || (k.forced_halo != 3 && htiles256 * 5 >= (int64_t)k.cus * 3);
  const int hbm = !halo ? 0 : hbig && halo_pixels(256, a.W) <= 383 ? 256
                  : k.forced_halo != 2 && halo_pixels(128, a.W) <= 191 ? 128 : 0;
  if (splits > 1) {
    // the LDS-DMA kernel on 64-row tiles, whatever else the conv is eligible for
  } else if (post) {
    if (big) return p;  // the 256x256 tile has no post epilogue
  } else if (hbm) {
    f = Family::halo;
    p.BM = hbm;
    p.BN = 128;
    p.threads = hbm * 2;
    // N-major placement when the filter outgrows an XCD's L2 share (4 MiB).
    p.nmajor = (int64_t)Cout * KS * KS * C * 2 > ((int64_t)5 << 19) ? 1 : 0;
  } else if (big) {
    f = Family::big;
    p.BM = p.BN = 256;
    p.threads = 512;
  } else if (narrow) {
    p.BN = 64;
    p.CSM = 16;
  } else if (pro && C <= 2048 && ktiles > 2 && Cout > 64 && (KS != 1 || a.pad == 0)) {
    // Short K (≤ 2 steps) or 64-wide outputs: the persistent register kernel,
    // which overlaps the next tile's loads with this tile's epilogue, wins there.
    // (conv_pro's 1x1 form assumes no padding: it skips the zero-padding select.)
    f = Family::pro;
  }
  // otherwise: LDS-DMA kernels for every conv without a prologue; the prologue convs
  // that conv_pro_kernel does not take stage A through registers (conv_gemm_kernel).
  p.family = f;
  p.nM = (M + p.BM - 1) / p.BM;
  p.nN = Cout / p.BN;
  return p;
}

// conv23 (conv2 3x3 + conv3 1x1 + residual in one kernel, C = 64 / 128): the rows
// per workgroup of conv23_kernel<BM, C, NEXT, 3, 256, POST, SC> on ceil(M / BM)
// workgroups, 0 for a variant that does not exist.  next: the following block's
// conv1 too; post: the post epilogue; sc: the projection shortcut in the tail.
constexpr int conv23_bm(int C, bool next, bool post, bool sc) {
  if ((C != 64 && C != 128) || (post && next) || (sc && (!next || C != 64))) return 0;
  return C == 64 ? 128 : 64;
}

// conv23's halo form of phase 1 (conv23_kernel<..., HALO>, stride 1): the region the
// 3-stage ring of (A tile + weight panel) occupies holds, per 64-channel block, one
// 128-B row per input pixel of the flat range [m0 − W − 1, m0 + BM + W + 1) that a
// tile of BM consecutive output pixels reads -- BM + 2W + 2 rows, all nine taps read
// their A fragments from it -- with the block's last row a zero row (padding taps
// and rows past M), and behind the halo a ring of `conv23_halo_ring` weight panels
// (C rows x 128 B).  Rows are DMA'd 32 at a time, so the row count is a multiple of 32.
constexpr int conv23_region(int C, int bm) { return 3 * (bm + C) * 128; }  // the ring form's LDS region, bytes
constexpr int conv23_halo_ring(int C) { return C == 64 ? 4 : 2; }          // weight panels in the halo form's ring
constexpr int conv23_halo_rows(int C, int bm) {  // halo rows per 64-channel block, the zero row included
  return (conv23_region(C, bm) - conv23_halo_ring(C) * C * 128) / 128 / (C / 64) / 32 * 32;
}
constexpr int conv23_halo_bytes(int C, int bm) {  // halo image + weight ring
  return conv23_halo_rows(C, bm) * (C / 64) * 128 + conv23_halo_ring(C) * C * 128;
}
// Whether a W-wide image runs the halo form: stride 1, C = 64, and the tile's halo
// rows plus the zero row fit (W ≤ 94: the flagship's 87 does).  Anything else keeps
// the ring.  C = 128 is not taken: there the region leaves a ring of two 16 KB panels,
// and on the flagship's 44-wide stage 2 the form gained 3-6 us per tail, inside the
// ring form's own round-to-round spread (profiles/r11/tail_halo), so it was not kept.
constexpr bool conv23_halo_ok(int C, int stride, int W, int bm) {
  if (stride != 1 || C != 64 || W < 1 || bm < 1 || bm % 32) return false;
  return (int64_t)bm + 2 * (int64_t)W + 3 <= conv23_halo_rows(C, bm);
}

}  // namespace convplan
