// Band plan of the fused stem kernel (stem_pool_kernel in conv_gemm.hip): which
// pooled rows of which image a workgroup walks.  Plain C++17, no HIP:
// tests/test_stem_plan_cpu.py compiles it with g++; the kernel calls
// stem_band() itself, so host, device and test share one definition.
//
// A band is the pooled rows [p0, p1) of one image.  Its first step computes
// the three stem rows 2*p0-1 .. 2*p0+1, every later step only the two new ones
// (row 2*pi-1 is still in the kernel's LDS row buffers), so a band of r pooled
// rows costs 2r + 1 stem rows and one stem row per band is computed twice.
// Every image is cut into bands of `rows` pooled rows, the last one shorter.
//
// The rule: LDS admits one workgroup per CU, so with nb = N * bands-per-image
// bands the busiest workgroup walks ceil(nb / cus) of them and the kernel takes
// about ceil(nb / cus) * (2 * rows + 1) stem rows of time.  The plan takes the
// band count per image that minimises this, the smaller count on a tie (less
// recompute).  Fewer, longer bands recompute less but leave CUs idle; more,
// shorter ones fill the CUs but pay the extra row more often, and past one
// wave of workgroups a second round costs a whole band.  At N = 50, PH = 87 on
// 256 CUs that is 5 bands of 18/18/18/18/15 rows: 250 workgroups in one wave,
// 37 stem rows each where one pooled row per task costs 17 tasks x 3 = 51, and
// the recompute is 1 row in 2 * 17.4 + 1.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define STEMPLAN_HD __host__ __device__
#else
#define STEMPLAN_HD
#endif

namespace stemplan {

struct StemPlan {
  int rows = 0;       // pooled rows per band (the last band of an image may have fewer)
  int per_image = 0;  // bands per image = ceil(PH / rows)
  int nbands = 0;     // N * per_image; 0: no plan (bad arguments or more than INT32_MAX bands)
  int grid = 0;       // workgroups = min(cus, nbands); workgroup g walks bands g, g + grid, ...
};

struct StemBand {
  int n, p0, p1;  // image, pooled rows [p0, p1)
};

// forced: 0 = the rule above, k > 0 = bands of k pooled rows (1: one pooled row
// per band, the decomposition before bands existed).
inline StemPlan stem_band_plan(int N, int PH, int cus, int forced) {
  StemPlan p;
  if (N < 1 || PH < 1 || cus < 1 || forced < 0) return p;
  int rows = PH;
  if (forced > 0) {
    rows = forced < PH ? forced : PH;
  } else {
    // the search stops at 4 bands per CU: it runs per launch, and bands that short mostly pay
    // their extra row
    const int most = PH < 4 * cus ? PH : 4 * cus;
    int64_t best = -1;
    for (int b = 1; b <= most; ++b) {
      const int r = (PH + b - 1) / b;
      const int64_t nb = (int64_t)N * ((PH + r - 1) / r);
      const int64_t cost = ((nb + cus - 1) / cus) * (2 * (int64_t)r + 1);
      if (best < 0 || cost < best) best = cost, rows = r;
    }
  }
  const int per_image = (PH + rows - 1) / rows;
  const int64_t nb = (int64_t)N * per_image;
  if (nb > INT32_MAX) return p;
  p.rows = rows;
  p.per_image = per_image;
  p.nbands = (int)nb;
  p.grid = nb < cus ? (int)nb : cus;
  return p;
}

STEMPLAN_HD inline StemBand stem_band(const StemPlan& p, int PH, int b) {
  const int n = b / p.per_image, p0 = (b - n * p.per_image) * p.rows;
  return {n, p0, p0 + p.rows < PH ? p0 + p.rows : PH};
}

}  // namespace stemplan
