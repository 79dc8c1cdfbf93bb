// Crop + bilinear resize of detections out of a full uint8 frame, on the GPU -- the input side of the two-stage pipeline.
//
// Replaces, for the batched regression stage, the reference's per-detection host loop
//   crop = frame[y0:y1, x0:x1]                      (utils/ie_wrappers.py:154-158, dataloaders/objectron_main.py:98-127)
//   cv.resize(crop, (w, h))                          (utils/ie_wrappers.py:18-21; albumentations Resize in the loaders)
// with one launch over all detections of a frame: frame [H,W,3] uint8 -> crops [n,oh,ow,3] uint8 NHWC, which the stem's
// patch gather (t3d_stem_im2col_u8) normalises and consumes as they are.
//
// Arithmetic: cv::resize's INTER_LINEAR for 8-bit images restated (csrc/resize_linear.h; parity with cv2 itself is UNPINNED,
// oracle/crop_resize.py is the same restatement in numpy and the kernel is bit-exact against it).
#include <hip/hip_runtime.h>

#include "common.h"
#include "resize_linear.h"

namespace {

__global__ __launch_bounds__(256) void crop_resize_kernel(const unsigned char* __restrict__ frame, const int* __restrict__ rects,
                                                          unsigned char* __restrict__ out, int n, int H, int W, int oh, int ow) {
  const size_t total = (size_t)n * oh * ow;
  for (size_t p = blockIdx.x * (size_t)256 + threadIdx.x; p < total; p += (size_t)gridDim.x * 256) {
    const int dx = (int)(p % ow), dy = (int)((p / ow) % oh), i = (int)(p / ((size_t)ow * oh));
    // numpy slicing of the reference: frame[y0:y1, x0:x1] with the bounds clamped to the frame
    const int x0 = min(max(rects[4 * i], 0), W), y0 = min(max(rects[4 * i + 1], 0), H);
    const int x1 = min(max(rects[4 * i + 2], 0), W), y1 = min(max(rects[4 * i + 3], 0), H);
    const int sw = x1 - x0, sh = y1 - y0;
    unsigned char* o = out + p * 3;
    if (sw <= 0 || sh <= 0) {      // empty crop (cv.resize would raise): zeros, the caller drops such detections
      o[0] = o[1] = o[2] = 0;
      continue;
    }
    const T3dLin cx = lin_coef(dx, sw, ow, true), cy = lin_coef(dy, sh, oh, false);
    const unsigned char* r0 = frame + ((size_t)(y0 + cy.i0) * W + x0) * 3;
    const unsigned char* r1 = frame + ((size_t)(y0 + cy.i1) * W + x0) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int d0 = r0[cx.i0 * 3 + c] * cx.w0 + r0[cx.i1 * 3 + c] * cx.w1;
      const int d1 = r1[cx.i0 * 3 + c] * cx.w0 + r1[cx.i1 * 3 + c] * cx.w1;
      o[c] = (unsigned char)lin_vert(d0, d1, cy);
    }
  }
}

}  // namespace

extern "C" int t3d_crop_resize_u8(const unsigned char* frame, const int* rects, unsigned char* out, int n, int H, int W, int oh,
                                  int ow, void* stream) {
  if (!frame || !rects || !out || n < 0 || H <= 0 || W <= 0 || oh <= 0 || ow <= 0) return T3D_ERR_ARG;
  if (n == 0) return T3D_OK;
  const size_t total = (size_t)n * oh * ow;
  const int grid = (int)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
  T3D_LAUNCH(crop_resize_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), frame, rects, out, n, H,
                     W, oh, ow);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
