// t3d_detect_roi_plan: between t3d_detect_draw and t3d_jpeg_decode_roi_u8, ONE launch that turns the drawn records of a
// detection batch into the rectangle decode's tables -- which part of each frame its crop reads, the MCU rectangle and segment
// run of that part, the item, the record rewritten for the sub-frame -- with nothing read back
// (torchdet3d/dataloaders/detection_arena.py, crop_decode).  csrc/detect_roi.h is the arithmetic; include/t3d.h states the
// contract; csrc/detect_roi_host.hip is the same on the CPU.
//
// Samples are independent and a sample is a few dozen integer operations, so a lane takes a sample: no scan, no atomics, no
// LDS.  A batch is one or two waves; the launch costs its latency.
#include "common.h"
#include "detect_roi.h"

namespace {

namespace P = t3d_roi;
static_assert(sizeof(t3d_det_sample) == 80 && sizeof(t3d_jpeg_item) == 48, "include/t3d.h");

__global__ __launch_bounds__(64) void detect_roi_plan_kernel(void* records, int B, const int* __restrict__ sample,
                                                             const t3d_jpeg_info* __restrict__ infos,
                                                             const t3d_jpeg_item* __restrict__ items, int n, long long src_bytes,
                                                             t3d_jpeg_item* __restrict__ roi_items, int* __restrict__ rects,
                                                             int* __restrict__ diag) {
  const int j = blockIdx.x * 64 + threadIdx.x;
  if (j >= n) return;
  P::plan_item(j, records, B, sample, infos, items, src_bytes, roi_items, rects, diag);
}

}  // namespace

extern "C" int t3d_detect_roi_plan(void* records, int B, const int* sample, const t3d_jpeg_info* infos, const t3d_jpeg_item* items,
                                   int n, long long src_bytes, t3d_jpeg_item* roi_items, int* rects, int* diag, void* stream) {
  const int rc = P::check(records, B, infos, items, n, src_bytes, roi_items, rects, diag);
  if (rc != T3D_OK || n == 0) return rc;
  T3D_LAUNCH(detect_roi_plan_kernel, dim3((n + 63) / 64), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), records, B, sample, infos,
             items, n, src_bytes, roi_items, rects, diag);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
