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
// template (aug_pixel) instantiated over the crop (CropSrc: four source pixels per resized pixel) and over the arena
// (ArenaSrc: a load), so the two entry points cannot drift apart.  A sample that is not rotated is a byte stream through
// the LUT there: 12 bytes per lane through aligned dword loads; a rotated pixel reads 4 arena taps instead of 16 crop taps.
#include <hip/hip_runtime.h>

#include "common.h"
#include "resize_linear.h"

namespace {

constexpr int AUG_PIX = 4;       // pixels per thread: 12 bytes -> three dword stores

__device__ __forceinline__ int lut_u8(int v, int lut, float alpha, float beta255) {
  if (lut) {
    const float t = __fadd_rn(__fmul_rn((float)v, alpha), beta255);
    v = (int)fminf(fmaxf(t, 0.f), 255.f);
  }
  return v;
}

// Where the resized image I(u, v) (before the flip and the LUT) comes from.  The two kernels differ in this and in nothing
// else: `row(v)` prepares a row, `px(row, u, out)` yields one pixel of it.

// the crop itself: I(u, v) is computed from its four source pixels (cv::resize INTER_LINEAR, csrc/resize_linear.h)
struct CropSrc {
  const unsigned char* crop;
  int h, w, oh, ow;
  typedef T3dLin Row;
  __device__ __forceinline__ bool init(const unsigned char* __restrict__ src, long long src_bytes, const t3d_aug_sample& s,
                                       int oh_, int ow_) {
    if (s.h <= 0 || s.w <= 0 || s.offset < 0 || s.offset + (long long)s.h * s.w * 3 > src_bytes) return false;
    crop = src + s.offset;
    h = s.h, w = s.w, oh = oh_, ow = ow_;
    return true;
  }
  __device__ __forceinline__ Row row(int v) const { return lin_coef(v, h, oh, false); }
  __device__ __forceinline__ void px(const Row& cy, int u, int out[3]) const {
    const T3dLin cx = lin_coef(u, w, ow, true);
    const unsigned char* r0 = crop + (size_t)cy.i0 * w * 3;
    const unsigned char* r1 = crop + (size_t)cy.i1 * w * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int d0 = r0[cx.i0 * 3 + c] * cx.w0 + r0[cx.i1 * 3 + c] * cx.w1;
      const int d1 = r1[cx.i0 * 3 + c] * cx.w0 + r1[cx.i1 * 3 + c] * cx.w1;
      out[c] = lin_vert(d0, d1, cy);
    }
  }
};

// an arena of images that were resized once: I(u, v) is a load (64-bit offsets: an arena holds a whole dataset)
struct ArenaSrc {
  const unsigned char* img;
  int ow;
  typedef const unsigned char* Row;
  __device__ __forceinline__ bool init(const unsigned char* __restrict__ arena, long long arena_bytes, const t3d_aug_sample& s,
                                       int oh_, int ow_) {
    const long long bytes = (long long)oh_ * ow_ * 3;
    if (s.h != oh_ || s.w != ow_ || s.offset < 0 || s.offset > arena_bytes - bytes) return false;
    img = arena + s.offset;
    ow = ow_;
    return true;
  }
  __device__ __forceinline__ Row row(int v) const { return img + (long long)v * ow * 3; }
  __device__ __forceinline__ void px(const Row& r, int u, int out[3]) const {
#pragma unroll
    for (int c = 0; c < 3; ++c) out[c] = r[u * 3 + c];
  }
};

__device__ __forceinline__ int u_src(int u, int ow, bool flip) { return flip ? ow - 1 - u : u; }

// one output pixel: flip, LUT, rotate and channel swap over the resized image `Src` yields
template <class Src>
__device__ __forceinline__ void aug_pixel(const unsigned char* __restrict__ src, long long src_bytes, const t3d_aug_sample& s,
                                          int dx, int dy, int oh, int ow, int px[3]) {
  px[0] = px[1] = px[2] = 0;
  Src img;
  if (!img.init(src, src_bytes, s, oh, ow)) return;   // bad record: zeros
  const bool flip = s.flags & T3D_AUG_FLIP;
  const int lut = s.flags & T3D_AUG_LUT;
  if (!(s.flags & T3D_AUG_ROTATE)) {
    img.px(img.row(dy), u_src(dx, ow, flip), px);
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = lut_u8(px[c], lut, s.alpha, s.beta255);
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
      const typename Src::Row row = img.row(v);
#pragma unroll
      for (int ax = 0; ax < 2; ++ax) {
        const int u = sx + ax;
        if (u < 0 || u >= ow) continue;
        int t[3];
        img.px(row, u_src(u, ow, flip), t);
        const int wt = wy[ay] * wx[ax] * 32;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += lut_u8(t[c], lut, s.alpha, s.beta255) * wt;
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

// pixels p0 .. p0 + n - 1 of the batch (they may belong to two samples), packed into three dwords
template <class Src>
__device__ __forceinline__ void aug_words(const unsigned char* __restrict__ src, long long src_bytes,
                                          const t3d_aug_sample* __restrict__ samples, long long p0, int n, long long plane,
                                          int oh, int ow, unsigned int word[3]) {
  word[0] = word[1] = word[2] = 0u;
#pragma unroll
  for (int k = 0; k < AUG_PIX; ++k) {
    if (k >= n) break;
    const long long p = p0 + k;
    const int i = (int)(p / plane), r = (int)(p - (long long)i * plane);
    const t3d_aug_sample s = samples[i];
    int px[3];
    aug_pixel<Src>(src, src_bytes, s, r % ow, r / ow, oh, ow, px);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int b = 3 * k + c;
      word[b >> 2] |= (unsigned int)px[c] << (8 * (b & 3));
    }
  }
}

__device__ __forceinline__ void store_words(unsigned char* __restrict__ out, long long p0, int n, const unsigned int word[3]) {
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
