// C ABI over native/kernels/conv_plan.h for tests/test_conv_plan_cpu.py (g++, no HIP).
#include "../kernels/conv_plan.h"

using namespace convplan;

namespace {
// The members of conv_gemm.hip's ConvArgs that conv_plan() reads.
struct Req {
  int N, H, W, C, Cout, stride, pad, act, res_stride;
  const void *pscale, *res, *bias, *stats, *bnx, *qscale, *gmask, *ws;
};
// shape: N H W C Cout KS stride pad act bias pro res stats res_stride post masked has_ws ws_bytes
Req req_of(const int64_t* v) {
  static const int there = 0;
  const auto ptr = [](bool on) { return on ? &there : nullptr; };
  return {(int)v[0], (int)v[1], (int)v[2],  (int)v[3],      (int)v[4],      (int)v[6],   (int)v[7],   (int)v[8], (int)v[13],
          ptr(v[10]), ptr(v[11]), ptr(v[9]), ptr(v[12] != 0), ptr(v[12] == 2), ptr(v[14]), ptr(v[15]), ptr(v[16])};
}
// knobs: cus forced_bm forced_big forced_halo forced_split env_big env_halo env_1x1_big
ConvKnobs knobs_of(const int64_t* v) {
  return {(int)v[0], (int)v[1], (int)v[2], (int)v[3], (int)v[4], (int)v[5], v[6] != 0, v[7] != 0};
}
}  // namespace

// out: family nb KS BM BN CSM ST threads RES POST splits kper nM nN nmajor past_split
extern "C" void conv_plan_c(const int64_t* shape, const int64_t* knobs, int last, int64_t* out) {
  const ConvPlan p = conv_plan(req_of(shape), (int)shape[5], shape[17], knobs_of(knobs), last != 0);
  const int64_t v[16] = {(int64_t)p.family, p.nb, p.KS, p.BM, p.BN, p.CSM, p.ST, p.threads, p.RES, p.POST,
                         p.splits, p.kper, p.nM, p.nN, p.nmajor, p.past_split()};
  for (int i = 0; i < 16; ++i) out[i] = v[i];
}

extern "C" int64_t conv_workspace_c(const int64_t* shape, const int64_t* knobs) {
  return conv_workspace((int)shape[0], (int)shape[1], (int)shape[2], (int)shape[3], (int)shape[4], (int)shape[5],
                        (int)shape[6], (int)shape[7], shape[10] != 0, knobs_of(knobs));
}

extern "C" int conv23_bm_c(int C, int next, int post, int sc) { return conv23_bm(C, next != 0, post != 0, sc != 0); }
