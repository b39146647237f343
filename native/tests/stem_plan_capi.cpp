// C ABI over native/kernels/stem_plan.h for tests/test_stem_plan_cpu.py (g++, no HIP).
#include "../kernels/stem_plan.h"

using namespace stemplan;

// out: rows per_image nbands grid
extern "C" void stem_band_plan_c(int N, int PH, int cus, int forced, int* out) {
  const StemPlan p = stem_band_plan(N, PH, cus, forced);
  out[0] = p.rows; out[1] = p.per_image; out[2] = p.nbands; out[3] = p.grid;
}

// Band b of the plan (as the kernel asks for it): out = n p0 p1
extern "C" void stem_band_c(int N, int PH, int cus, int forced, int b, int* out) {
  const StemBand s = stem_band(stem_band_plan(N, PH, cus, forced), PH, b);
  out[0] = s.n; out[1] = s.p0; out[2] = s.p1;
}

// Every band of the plan at once: out[3 * b ..] = n p0 p1; returns nbands (out may be null).
extern "C" int stem_bands_c(int N, int PH, int cus, int forced, int* out) {
  const StemPlan p = stem_band_plan(N, PH, cus, forced);
  for (int b = 0; out && b < p.nbands; ++b) {
    const StemBand s = stem_band(p, PH, b);
    out[3 * b] = s.n; out[3 * b + 1] = s.p0; out[3 * b + 2] = s.p1;
  }
  return p.nbands;
}
