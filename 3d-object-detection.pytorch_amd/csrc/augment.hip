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
//
// t3d_augment_resized_u8 is the same pipeline over an arena of crops that were resized once (this kernel with no flag
// set): the reference decodes, crops and resizes every object again in every epoch (`Objectron.__getitem__` + A.Resize,
// dataloaders/objectron_main.py:51-96), although resize(crop(frame)) never changes.  Everything after the resize is one
// template (aug_pixel, csrc/augment_pixel.h: shared with csrc/augment_chain.hip, the pipelines with random_rescale,
// hue_saturation_value or color_jitter) instantiated over the crop (CropSrc: four source pixels per resized pixel) and over the arena
// (ArenaSrc: a load), so the two entry points cannot drift apart.  A sample that is not rotated is a byte stream through
// the LUT there: 12 bytes per lane through aligned dword loads; a rotated pixel reads 4 arena taps instead of 16 crop taps.
#include <hip/hip_runtime.h>

#include "augment_pixel.h"

namespace {

__global__ __launch_bounds__(256) void augment_crops_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                            const t3d_aug_sample* __restrict__ samples,
                                                            unsigned char* __restrict__ out, int B, int oh, int ow) {
  const long long npix = (long long)B * oh * ow, plane = (long long)oh * ow;
  const long long nthr = (npix + AUG_PIX - 1) / AUG_PIX;
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < nthr; t += (long long)gridDim.x * 256) {
    const long long p0 = t * AUG_PIX;
    const int n = (int)min((long long)AUG_PIX, npix - p0);
    unsigned int word[3];
    aug_words<CropSrc>(src, src_bytes, samples, p0, n, plane, oh, ow, word);
    store_words(out, p0, n, word);
  }
}

// 12 bytes at any alignment through aligned dword loads.  A misaligned run of 12 bytes touches four aligned dwords and each
// of them holds at least one byte of the run, so nothing is read from a dword (hence a page) the run does not reach.
__device__ __forceinline__ void load12(const unsigned char* __restrict__ p, unsigned int w[3]) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const unsigned int* q = reinterpret_cast<const unsigned int*>(a & ~(uintptr_t)3);
  const unsigned int sh = 8u * (unsigned int)(a & 3);
  if (sh == 0) {
    w[0] = q[0];
    w[1] = q[1];
    w[2] = q[2];
  } else {
    const unsigned int x0 = q[0], x1 = q[1], x2 = q[2], x3 = q[3];
    w[0] = (x0 >> sh) | (x1 << (32 - sh));
    w[1] = (x1 >> sh) | (x2 << (32 - sh));
    w[2] = (x2 >> sh) | (x3 << (32 - sh));
  }
}

// Four pixels of one sample that is not rotated: the arena bytes are the output bytes but for the order of the pixels
// (flip), the LUT and the order of the channels.  false: the pixels are not one run of a row (the caller goes per pixel).
__device__ __forceinline__ bool stream_words(const ArenaSrc& img, const t3d_aug_sample& s, int r, int ow, unsigned int word[3]) {
  const bool flip = s.flags & T3D_AUG_FLIP;
  long long first = r;                             // the source pixel with the lowest address
  if (flip) {
    const int dy = r / ow, dx = r - dy * ow;
    if (dx + AUG_PIX > ow) return false;           // a flipped run must stay within its row
    first = (long long)dy * ow + (ow - AUG_PIX - dx);
  }
  unsigned int w[3];
  load12(img.img + first * 3, w);
  const int lut = s.flags & T3D_AUG_LUT;
  const bool swap = s.flags & T3D_AUG_SWAP_RB;
  word[0] = word[1] = word[2] = 0u;
#pragma unroll
  for (int k = 0; k < AUG_PIX; ++k) {
    const int ks = flip ? AUG_PIX - 1 - k : k;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int bs = 3 * ks + (swap ? 2 - c : c), b = 3 * k + c;
      const int v = lut_u8((int)((w[bs >> 2] >> (8 * (bs & 3))) & 255u), lut, s.alpha, s.beta255);
      word[b >> 2] |= (unsigned int)v << (8 * (b & 3));
    }
  }
  return true;
}

__global__ __launch_bounds__(256) void augment_resized_kernel(const unsigned char* __restrict__ arena, long long arena_bytes,
                                                              const t3d_aug_sample* __restrict__ samples,
                                                              unsigned char* __restrict__ out, int B, int oh, int ow) {
  const long long npix = (long long)B * oh * ow, plane = (long long)oh * ow;
  const long long nthr = (npix + AUG_PIX - 1) / AUG_PIX;
  for (long long t = blockIdx.x * 256ll + threadIdx.x; t < nthr; t += (long long)gridDim.x * 256) {
    const long long p0 = t * AUG_PIX;
    const int n = (int)min((long long)AUG_PIX, npix - p0);
    unsigned int word[3];
    bool done = false;
    const int i = (int)(p0 / plane), r = (int)(p0 - (long long)i * plane);
    if (n == AUG_PIX && r + AUG_PIX <= plane) {    // four pixels of one sample
      const t3d_aug_sample s = samples[i];
      ArenaSrc img;
      if (!img.init(arena, arena_bytes, s, oh, ow)) {
        word[0] = word[1] = word[2] = 0u;          // bad record: zeros
        done = true;
      } else if (!(s.flags & T3D_AUG_ROTATE)) {
        done = stream_words(img, s, r, ow, word);
      }
    }
    if (!done) aug_words<ArenaSrc>(arena, arena_bytes, samples, p0, n, plane, oh, ow, word);
    store_words(out, p0, n, word);
  }
}

int launch_grid(int B, int oh, int ow) {
  const long long nthr = ((long long)B * oh * ow + AUG_PIX - 1) / AUG_PIX;
  return (int)((nthr + 255) / 256 > 16384 ? 16384 : (nthr + 255) / 256);
}

}  // namespace

extern "C" int t3d_augment_crops_u8(const unsigned char* src, long long src_bytes, const void* samples, unsigned char* out, int B,
                                    int oh, int ow, void* stream) {
  if (!src || !samples || !out || src_bytes <= 0 || B < 0 || oh <= 0 || ow <= 0 || (reinterpret_cast<uintptr_t>(out) & 3))
    return T3D_ERR_ARG;
  if (B == 0) return T3D_OK;
  T3D_LAUNCH(augment_crops_kernel, dim3(launch_grid(B, oh, ow)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), src,
             src_bytes, reinterpret_cast<const t3d_aug_sample*>(samples), out, B, oh, ow);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_augment_resized_u8(const unsigned char* arena, long long arena_bytes, const void* samples, unsigned char* out,
                                      int B, int oh, int ow, void* stream) {
  if (!arena || !samples || !out || arena_bytes <= 0 || B < 0 || oh <= 0 || ow <= 0 || (reinterpret_cast<uintptr_t>(out) & 3))
    return T3D_ERR_ARG;
  if (B == 0) return T3D_OK;
  T3D_LAUNCH(augment_resized_kernel, dim3(launch_grid(B, oh, ow)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arena,
             arena_bytes, reinterpret_cast<const t3d_aug_sample*>(samples), out, B, oh, ow);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
