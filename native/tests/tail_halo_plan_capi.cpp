// C ABI over conv_plan.h's conv23 halo rule for tests/test_tail_halo_plan_cpu.py (g++, no HIP).
#include "../kernels/conv_plan.h"

using namespace convplan;

extern "C" int conv23_halo_ok_c(int C, int stride, int W, int bm) { return conv23_halo_ok(C, stride, W, bm); }
extern "C" int conv23_halo_rows_c(int C, int bm) { return conv23_halo_rows(C, bm); }
extern "C" int conv23_halo_ring_c(int C) { return conv23_halo_ring(C); }
extern "C" int conv23_halo_bytes_c(int C, int bm) { return conv23_halo_bytes(C, bm); }
extern "C" int conv23_region_c(int C, int bm) { return conv23_region(C, bm); }
extern "C" int conv23_bm_c(int C, int next, int post, int sc) { return conv23_bm(C, next != 0, post != 0, sc != 0); }
