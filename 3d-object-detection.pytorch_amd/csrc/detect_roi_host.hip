// t3d_detect_roi_plan_host: t3d_detect_roi_plan on the CPU -- the same arguments, host pointers, no HIP call -- which the CPU
// suite holds to numpy (tests/test_detect_roi_plan_host.py).
// A unit of its own because csrc/jpeg_decode.h, whose roi_mcus the planner includes, marks its functions __device__ when
// __HIPCC__ is defined: here the lane headers are read as the plain C++ they also are (tools/jpeg_index_check.cpp reads them so).
#undef __HIPCC__
#include "detect_roi.h"

extern "C" int t3d_detect_roi_plan_host(void* records, int B, const int* sample, const t3d_jpeg_info* infos, const t3d_jpeg_item* items,
                                        int n, long long src_bytes, t3d_jpeg_item* roi_items, int* rects, int* diag, void* stream) {
  (void)stream;
  const int rc = t3d_roi::check(records, B, infos, items, n, src_bytes, roi_items, rects, diag);
  if (rc != T3D_OK) return rc;
  for (int j = 0; j < n; ++j) t3d_roi::plan_item(j, records, B, sample, infos, items, src_bytes, roi_items, rects, diag);
  return T3D_OK;
}
