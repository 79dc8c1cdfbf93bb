// The per-pixel half of the crop augmentations, shared by csrc/augment.hip and csrc/augment_chain.hip: where the resized
// image comes from (CropSrc / ArenaSrc), the brightness / contrast LUT, one output pixel of flip -> LUT -> warp -> channel
// swap (aug_pixel), and the 4-pixel word packing.  The arithmetic is described at the top of csrc/augment.hip.
#pragma once
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

}  // namespace
