// The reference's training augmentations on a batch of Objectron crops, one launch per batch.
//
// Replaces the host pipeline that `Objectron.__getitem__` runs on each cropped object (dataloaders/objectron_main.py:71-80,
// builders/loader_builder.py:38-68, configs/default_config.py:31-37):
//   A.Resize -> A.HorizontalFlip -> A.RandomBrightnessContrast -> RandomRotate (utils/transforms.py:50-89) -> [ConvertColor]
// crops of different sizes packed in one uint8 buffer -> out [B, oh, ow, 3] uint8 NHWC, which the stem's patch gather
// (t3d_stem_im2col_u8) normalises as it is.  Each output pixel is a pure function of a few crop pixels, computed on the fly
// with the reference's 8-bit rounding points (uint8 after the resize and after the LUT); no LDS, no atomics.
//
// Arithmetic (OpenCV / albumentations are not dependencies: parity with them is UNPINNED; tests/augment_ref.py restates
// the same steps in numpy and the kernel is bit-exact against it):
//   resize    cv::resize INTER_LINEAR, 8-bit (csrc/resize_linear.h -- t3d_crop_resize_u8's arithmetic)
//   flip      u -> ow - 1 - u on the resized image
//   LUT       lut[i] = (uint8) clip(float32(i) * alpha + beta255, 0, 255)  in float32, truncated (albumentations
//             brightness_contrast_adjust on uint8, brightness_by_max = True)
//   rotate    cv::warpAffine INTER_LINEAR, BORDER_CONSTANT 0, OpenCV's fixed-point path: the record holds the INVERSE map
//             m (dst -> src, as warpAffine inverts getRotationMatrix2D's matrix, in fp64);
//               X0 = cvRound((m1*y + m2) * 1024) + 16,  adelta = cvRound(m0*x * 1024)    (AB_BITS = 10, round half even)
//               X = (X0 + adelta) >> 5, sx = X >> 5, fx = X & 31   (INTER_BITS = 5; Y likewise with m3, m4, m5)
//               out = (sum of the four taps * (32-fy|fy)*(32-fx|fx)*32 + 2^14) >> 15, taps outside the image are 0
//             (INTER_REMAP_COEF_BITS = 15; OpenCV stores the (0,0) weight as 32767, which gives the same byte)
//   swap      RGB -> BGR when the pipeline has no convert_color
#include <hip/hip_runtime.h>

#include "common.h"
#include "resize_linear.h"

namespace {

constexpr int AUG_PIX = 4;       // pixels per thread: 12 bytes -> three dword stores

struct Taps { T3dLin c[2], r[2]; };

// one pixel of the resized (and flipped) crop, through the LUT: I2(u, v) with precomputed coefficients
__device__ __forceinline__ void resized_px(const unsigned char* __restrict__ crop, int w, const T3dLin& cx, const T3dLin& cy,
                                           int lut, float alpha, float beta255, int px[3]) {
  const unsigned char* r0 = crop + (size_t)cy.i0 * w * 3;
  const unsigned char* r1 = crop + (size_t)cy.i1 * w * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int d0 = r0[cx.i0 * 3 + c] * cx.w0 + r0[cx.i1 * 3 + c] * cx.w1;
    const int d1 = r1[cx.i0 * 3 + c] * cx.w0 + r1[cx.i1 * 3 + c] * cx.w1;
    int v = lin_vert(d0, d1, cy);
    if (lut) {
      const float t = __fadd_rn(__fmul_rn((float)v, alpha), beta255);
      v = (int)fminf(fmaxf(t, 0.f), 255.f);
    }
    px[c] = v;
  }
}

__device__ __forceinline__ int u_src(int u, int ow, bool flip) { return flip ? ow - 1 - u : u; }

__device__ __forceinline__ void aug_pixel(const unsigned char* __restrict__ src, long long src_bytes,
                                          const t3d_aug_sample& s, int dx, int dy, int oh, int ow, int px[3]) {
  px[0] = px[1] = px[2] = 0;
  if (s.h <= 0 || s.w <= 0 || s.offset < 0 || s.offset + (long long)s.h * s.w * 3 > src_bytes) return;   // bad record: zeros
  const unsigned char* crop = src + s.offset;
  const bool flip = s.flags & T3D_AUG_FLIP;
  const int lut = s.flags & T3D_AUG_LUT;
  if (!(s.flags & T3D_AUG_ROTATE)) {
    const T3dLin cx = lin_coef(u_src(dx, ow, flip), s.w, ow, true), cy = lin_coef(dy, s.h, oh, false);
    resized_px(crop, s.w, cx, cy, lut, s.alpha, s.beta255, px);
  } else {
    const double* m = s.m;
    const int X0 = __double2int_rn((m[1] * dy + m[2]) * 1024.0) + 16;
    const int Y0 = __double2int_rn((m[4] * dy + m[5]) * 1024.0) + 16;
    const int X = (X0 + __double2int_rn(m[0] * dx * 1024.0)) >> 5;
    const int Y = (Y0 + __double2int_rn(m[3] * dx * 1024.0)) >> 5;
    const int sx = min(max(X >> 5, -32768), 32767), sy = min(max(Y >> 5, -32768), 32767);   // saturate_cast<short>
    const int fx = X & 31, fy = Y & 31;
    const int wx[2] = {32 - fx, fx}, wy[2] = {32 - fy, fy};
    int acc[3] = {0, 0, 0};
#pragma unroll
    for (int ay = 0; ay < 2; ++ay) {
      const int v = sy + ay;
      if (v < 0 || v >= oh) continue;
      const T3dLin cy = lin_coef(v, s.h, oh, false);
#pragma unroll
      for (int ax = 0; ax < 2; ++ax) {
        const int u = sx + ax;
        if (u < 0 || u >= ow) continue;
        const T3dLin cx = lin_coef(u_src(u, ow, flip), s.w, ow, true);
        int t[3];
        resized_px(crop, s.w, cx, cy, lut, s.alpha, s.beta255, t);
        const int wt = wy[ay] * wx[ax] * 32;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += t[c] * wt;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = min((acc[c] + (1 << 14)) >> 15, 255);
  }
  if (s.flags & T3D_AUG_SWAP_RB) {
    const int t = px[0];
    px[0] = px[2];
    px[2] = t;
  }
}

__global__ __launch_bounds__(256) void augment_crops_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                            const t3d_aug_sample* __restrict__ samples,
                                                            unsigned char* __restrict__ out, int B, int oh, int ow) {
  const long long npix = (long long)B * oh * ow, plane = (long long)oh * ow;
  const long long nthr = (npix + AUG_PIX - 1) / AUG_PIX;
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < nthr; t += (long long)gridDim.x * 256) {
    const long long p0 = t * AUG_PIX;
    const int n = (int)min((long long)AUG_PIX, npix - p0);
    unsigned int word[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < AUG_PIX; ++k) {
      if (k >= n) break;
      const long long p = p0 + k;
      const int i = (int)(p / plane), r = (int)(p - (long long)i * plane);
      const t3d_aug_sample s = samples[i];
      int px[3];
      aug_pixel(src, src_bytes, s, r % ow, r / ow, oh, ow, px);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int b = 3 * k + c;
        word[b >> 2] |= (unsigned int)px[c] << (8 * (b & 3));
      }
    }
    unsigned char* o = out + p0 * 3;
    if (n == AUG_PIX) {            // out + 12 t: dword aligned (the caller's buffer is)
      unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
      o4[0] = word[0];
      o4[1] = word[1];
      o4[2] = word[2];
    } else {
      for (int b = 0; b < 3 * n; ++b) o[b] = (unsigned char)(word[b >> 2] >> (8 * (b & 3)));
    }
  }
}

}  // namespace

extern "C" int t3d_augment_crops_u8(const unsigned char* src, long long src_bytes, const void* samples, unsigned char* out, int B,
                                    int oh, int ow, void* stream) {
  if (!src || !samples || !out || src_bytes <= 0 || B < 0 || oh <= 0 || ow <= 0 || (reinterpret_cast<uintptr_t>(out) & 3))
    return T3D_ERR_ARG;
  if (B == 0) return T3D_OK;
  const long long nthr = ((long long)B * oh * ow + AUG_PIX - 1) / AUG_PIX;
  const int grid = (int)((nthr + 255) / 256 > 16384 ? 16384 : (nthr + 255) / 256);
  T3D_LAUNCH(augment_crops_kernel, dim3(grid), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src, src_bytes,
             reinterpret_cast<const t3d_aug_sample*>(samples), out, B, oh, ow);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
