// The crop augmentations of a pipeline that names random_rescale, hue_saturation_value or color_jitter: the three
// transforms of the reference's TRANSFORMS_REGISTRY (builders/loader_builder.py:38-52; RandomRescale is
// utils/transforms.py:20-47) that csrc/augment.hip's single launch cannot hold -- a contrast factor needs the mean of the
// whole image, and two warps in a row round to uint8 between them.  The default pipeline never comes here.
//
// Per sample:  resize -> flip -> [base LUT] -> colour program (<= 8 ops, in the record's order) -> warp -> warp -> swap.
// Launches (t3d_augment_chain_crops_u8 / t3d_augment_chain_resized_u8, `stages` says which are needed):
//   1. chain_mean_kernel    only with T3D_STAGE_MEAN: per sample with a CONTRAST op, every resized pixel goes through the ops
//                           in front of it and its grey is summed -- 32-bit integer partials per lane, a wave reduction, one
//                           64-bit integer atomic per workgroup into the sample's slot (integer sums: order-independent,
//                           the loader stays bit-reproducible).  The slots are zeroed by a memset in front of the launch.
//   2. chain_colour_kernel  resize (or arena load) -> flip -> LUT -> the whole program.  Writes the output (with the channel
//                           swap) for a sample no warp fires on, else the uint8 image the first warp reads.
//   3. chain_warp_kernel    only with T3D_STAGE_WARP / T3D_STAGE_WARP2, once per stage: aug_pixel's warp over the previous
//                           pass's uint8 image (csrc/augment_pixel.h: the very code t3d_augment_resized_u8 rotates with).  An
//                           intermediate [B, oh, ow, 3] image costs 150 KB per sample and pass at 224 x 224; nesting the taps
//                           would read 4 x 4 x 4 crop pixels per output pixel and run the colour program 16 times.
// Both entry points are one template over the source image (CropSrc / ArenaSrc), so cached and uncached batches agree bit
// for bit.  A bad record gives a zero image: the colour pass writes the zeros where the sample's next pass reads.
//
// Arithmetic (recalled from the OpenCV 4.x / albumentations 1.x sources, neither of which is a dependency: parity with the
// libraries is UNPINNED; tests/augment_chain_ref.py restates the same steps in numpy and the kernels are bit-exact against it):
//   RGB -> HSV  8-bit, H in 0..179: v = max, diff = v - min, s = (diff * sdiv[v] + 2^11) >> 12,
//               h = v == r ? g - b : v == g ? b - r + 2 diff : r - g + 4 diff;  h = (h * hdiv[diff] + 2^11) >> 12 (arithmetic
//               shift), h += 180 if h < 0;  sdiv[i] = rint((255 << 12) / i), hdiv[i] = rint((180 << 12) / (6 i)), 0 at i = 0
//   HSV -> RGB  float32, every product and sum rounded on its own: hf = H * (6 / 180) (minus 6 while >= 6), s = S / 255,
//               v = V / 255, sector = floor(hf), f = hf - sector, tab = {v, v(1 - s), v(1 - s f), v(1 - s(1 - f))},
//               (b, g, r) = tab[{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}][sector], byte = rint(x * 255) half to even
//   HSV shift   H = (uint8) mod(H + dh, 180) (the divisor's sign, as numpy), S = (uint8) clip(S + ds, 0, 255), V likewise, fp64
//   grey        (9798 R + 19235 G + 3735 B + 2^14) >> 15
//   jitter      brightness lut[i] = (uint8) clip(i f, 0, 255), contrast lut[i] = (uint8) clip(i f + mean (1 - f), 0, 255), fp64;
//               saturation rint(float32(x) float32(f) + float32(grey) float32(1 - f)) saturated (cv::addWeighted, 8-bit);
//               hue = HSV shift by 180 f.  Contrast uses the general formula for every f (albumentations special-cases
//               exactly 0 and 1).
#include <hip/hip_runtime.h>

#include "augment_pixel.h"

namespace {

// rint(n / i), half to even, 0 at i = 0
struct ChainDivTab {
  int sdiv[256], hdiv[256];
  static constexpr int rdiv(int n, int d) {
    if (d == 0) return 0;
    const int q = n / d, r = n % d;
    return 2 * r > d ? q + 1 : (2 * r == d ? q + (q & 1) : q);
  }
  constexpr ChainDivTab() : sdiv(), hdiv() {
    for (int i = 0; i < 256; ++i) {
      sdiv[i] = rdiv(255 << 12, i);
      hdiv[i] = rdiv(180 << 12, 6 * i);
    }
  }
};
__constant__ ChainDivTab g_chain_div = ChainDivTab();

__device__ __forceinline__ int grey_u8(const int px[3]) { return (9798 * px[0] + 19235 * px[1] + 3735 * px[2] + (1 << 14)) >> 15; }

__device__ __forceinline__ void rgb_to_hsv(const int px[3], int hsv[3]) {
  const int r = px[0], g = px[1], b = px[2];
  const int v = max(max(r, g), b), diff = v - min(min(r, g), b);
  const int s = (diff * g_chain_div.sdiv[v] + (1 << 11)) >> 12;
  int h = v == r ? g - b : (v == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h * g_chain_div.hdiv[diff] + (1 << 11)) >> 12;
  if (h < 0) h += 180;
  hsv[0] = h, hsv[1] = s, hsv[2] = v;
}

__device__ __forceinline__ int unit_to_u8(float x) { return (int)fminf(fmaxf(rintf(__fmul_rn(x, 255.f)), 0.f), 255.f); }

__device__ __forceinline__ void hsv_to_rgb(const int hsv[3], int px[3]) {
  float hf = __fmul_rn((float)hsv[0], 6.f / 180.f);
  const float s = __fmul_rn((float)hsv[1], 1.f / 255.f), v = __fmul_rn((float)hsv[2], 1.f / 255.f);
  while (hf >= 6.f) hf = __fsub_rn(hf, 6.f);
  const float fl = floorf(hf);
  const int sector = (int)fl;
  const float f = __fsub_rn(hf, fl);
  float tab[4];
  tab[0] = v;
  tab[1] = __fmul_rn(v, __fsub_rn(1.f, s));
  tab[2] = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, f)));
  tab[3] = __fmul_rn(v, __fsub_rn(1.f, __fmul_rn(s, __fsub_rn(1.f, f))));
  // OpenCV's sector table, (b, g, r) per sector, two bits an entry
  const unsigned int bsel = 0x835u, gsel = 0x583u, rsel = 0x358u;      // b {1,1,3,0,0,2}, g {3,0,0,2,1,1}, r {0,2,1,1,3,0}
  const int sh = 2 * sector;
  float r = tab[0], g = tab[0], b = tab[0];
  const int ri = (rsel >> sh) & 3, gi = (gsel >> sh) & 3, bi = (bsel >> sh) & 3;
#pragma unroll
  for (int k = 1; k < 4; ++k) {
    r = ri == k ? tab[k] : r;
    g = gi == k ? tab[k] : g;
    b = bi == k ? tab[k] : b;
  }
  px[0] = unit_to_u8(r), px[1] = unit_to_u8(g), px[2] = unit_to_u8(b);
}

// numpy's mod for a positive divisor
__device__ __forceinline__ double mod180(double x) {
  double r = fmod(x, 180.0);
  if (r < 0.0) r += 180.0;
  return r;
}

__device__ __forceinline__ int clip_trunc_u8(double x) { return (int)fmin(fmax(x, 0.0), 255.0); }

__device__ __forceinline__ void hsv_shift(int px[3], double dh, double ds, double dv) {
  int hsv[3];
  rgb_to_hsv(px, hsv);
  hsv[0] = (int)mod180((double)hsv[0] + dh);                 // (0 .. 180: the sum can round up to the divisor)
  hsv[1] = clip_trunc_u8((double)hsv[1] + ds);
  hsv[2] = clip_trunc_u8((double)hsv[2] + dv);
  hsv_to_rgb(hsv, px);
}

// Is the program well formed, and where is its CONTRAST op (-1: none)?
__device__ __forceinline__ bool chain_check(const t3d_aug_sample& s, const t3d_aug_chain& e, int stages, int* contrast_at) {
  *contrast_at = -1;
  if (e.n_ops < 0 || e.n_ops > T3D_CHAIN_MAX_OPS || (e.flags & ~T3D_CHAIN_WARP2)) return false;
  for (int k = 0; k < e.n_ops; ++k) {
    if (e.kind[k] < T3D_CHAIN_LUT || e.kind[k] > T3D_CHAIN_HUE) return false;
    if (e.kind[k] == T3D_CHAIN_CONTRAST) {
      if (*contrast_at >= 0) return false;
      *contrast_at = k;
    }
  }
  const bool w1 = s.flags & T3D_AUG_ROTATE, w2 = e.flags & T3D_CHAIN_WARP2;
  if (w2 && !w1) return false;
  if ((*contrast_at >= 0 && !(stages & T3D_STAGE_MEAN)) || (w1 && !(stages & T3D_STAGE_WARP)) || (w2 && !(stages & T3D_STAGE_WARP2)))
    return false;
  return true;
}

// ops [0, upto) of the program on one pixel; `mean` is only read by a CONTRAST op
__device__ __forceinline__ void chain_run(int px[3], const t3d_aug_chain* __restrict__ e, int upto, double mean) {
  for (int k = 0; k < upto; ++k) {
    const double p0 = e->p[k][0];
    switch (e->kind[k]) {
      case T3D_CHAIN_LUT: {
        const float alpha = (float)p0, beta255 = (float)e->p[k][1];
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = lut_u8(px[c], 1, alpha, beta255);
        break;
      }
      case T3D_CHAIN_HSV: hsv_shift(px, p0, e->p[k][1], e->p[k][2]); break;
      case T3D_CHAIN_BRIGHTNESS:
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = clip_trunc_u8((double)px[c] * p0);
        break;
      case T3D_CHAIN_CONTRAST: {
        const double off = mean * (1.0 - p0);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = clip_trunc_u8((double)px[c] * p0 + off);
        break;
      }
      case T3D_CHAIN_SATURATION: {
        const float fa = (float)p0, fb = (float)(1.0 - p0);
        const float gb = __fmul_rn((float)grey_u8(px), fb);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = (int)fminf(fmaxf(rintf(__fadd_rn(__fmul_rn((float)px[c], fa), gb)), 0.f), 255.f);
        break;
      }
      case T3D_CHAIN_HUE: hsv_shift(px, 180.0 * p0, 0.0, 0.0); break;
      default: break;
    }
  }
}

// up to AUG_PIX pixels of ONE sample to `dst + first * 3`: dwords when the run is whole and the address allows it
__device__ __forceinline__ void store_run(unsigned char* __restrict__ dst, long long first, int n, const unsigned int word[3]) {
  unsigned char* o = dst + first * 3;
  if (n == AUG_PIX && !(reinterpret_cast<uintptr_t>(o) & 3)) {
    unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
    o4[0] = word[0], o4[1] = word[1], o4[2] = word[2];
  } else {
    for (int b = 0; b < 3 * n; ++b) o[b] = (unsigned char)(word[b >> 2] >> (8 * (b & 3)));
  }
}

__device__ __forceinline__ void pack_px(unsigned int word[3], int k, const int px[3], bool swap) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int b = 3 * k + c;
    word[b >> 2] |= (unsigned int)px[swap ? 2 - c : c] << (8 * (b & 3));
  }
}

// grid (x, B): the workgroups of row blockIdx.y share sample blockIdx.y's plane, AUG_PIX consecutive pixels per thread and round

template <class Src>
__global__ __launch_bounds__(256) void chain_mean_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                         const t3d_aug_sample* __restrict__ samples,
                                                         const t3d_aug_chain* __restrict__ chains,
                                                         unsigned long long* __restrict__ sums, int oh, int ow, int stages) {
  __shared__ unsigned int part[4];
  const int i = blockIdx.y, plane = oh * ow;
  const t3d_aug_sample s = samples[i];
  const t3d_aug_chain* e = chains + i;
  int at;
  Src img;
  if (!chain_check(s, *e, stages, &at) || at < 0 || !img.init(src, src_bytes, s, oh, ow)) return;      // (uniform per workgroup)
  const int lut = s.flags & T3D_AUG_LUT;
  unsigned int acc = 0;                        // <= 255 per pixel: 2^24 pixels per lane before it could wrap
  for (int r = blockIdx.x * 256 + threadIdx.x; r < plane; r += gridDim.x * 256) {
    int px[3];
    img.px(img.row(r / ow), r % ow, px);       // (the flip permutes the pixels of a row: the sum does not see it)
#pragma unroll
    for (int c = 0; c < 3; ++c) px[c] = lut_u8(px[c], lut, s.alpha, s.beta255);
    chain_run(px, e, at, 0.0);
    acc += (unsigned int)grey_u8(px);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long t = (unsigned long long)part[0] + part[1] + part[2] + part[3];
    if (t) atomicAdd(sums + i, t);
  }
}

template <class Src>
__global__ __launch_bounds__(256) void chain_colour_kernel(const unsigned char* __restrict__ src, long long src_bytes,
                                                           const t3d_aug_sample* __restrict__ samples,
                                                           const t3d_aug_chain* __restrict__ chains,
                                                           const unsigned long long* __restrict__ sums,
                                                           unsigned char* __restrict__ tmp, unsigned char* __restrict__ out,
                                                           int oh, int ow, int stages) {
  const int i = blockIdx.y, plane = oh * ow;
  const t3d_aug_sample s = samples[i];
  const t3d_aug_chain* e = chains + i;
  int at;
  Src img;
  const bool good = chain_check(s, *e, stages, &at);
  const bool ok = good && img.init(src, src_bytes, s, oh, ow);
  const bool to_tmp = good && (s.flags & T3D_AUG_ROTATE);         // a warp pass reads this sample (zeros, if its source is bad)
  const bool flip = s.flags & T3D_AUG_FLIP, swap = !to_tmp && (s.flags & T3D_AUG_SWAP_RB);
  const int lut = s.flags & T3D_AUG_LUT;
  const double mean = ok && at >= 0 ? (double)sums[i] / (double)plane : 0.0;
  unsigned char* dst = (to_tmp ? tmp : out) + (long long)i * plane * 3;
  const int nrun = (plane + AUG_PIX - 1) / AUG_PIX;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < nrun; t += gridDim.x * 256) {
    const int r0 = t * AUG_PIX, n = min(AUG_PIX, plane - r0);
    unsigned int word[3] = {0u, 0u, 0u};
    if (ok) {
#pragma unroll
      for (int k = 0; k < AUG_PIX; ++k) {
        if (k >= n) break;
        const int r = r0 + k;
        int px[3];
        img.px(img.row(r / ow), u_src(r % ow, ow, flip), px);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = lut_u8(px[c], lut, s.alpha, s.beta255);
        chain_run(px, e, e->n_ops, mean);
        pack_px(word, k, px, swap);
      }
    }
    store_run(dst, r0, n, word);
  }
}

// One warp stage over the uint8 images of the pass before it.  second == 0: `from` -> m of the base record -> `to` (the
// output, unless the sample has a second warp); second == 1: `from` -> m2 -> the output.
__global__ __launch_bounds__(256) void chain_warp_kernel(const t3d_aug_sample* __restrict__ samples,
                                                         const t3d_aug_chain* __restrict__ chains,
                                                         const unsigned char* __restrict__ from, unsigned char* __restrict__ to,
                                                         unsigned char* __restrict__ out, int B, int oh, int ow, int stages,
                                                         int second) {
  const int i = blockIdx.y, plane = oh * ow;
  const t3d_aug_sample s = samples[i];
  const t3d_aug_chain* e = chains + i;
  int at;
  if (!chain_check(s, *e, stages, &at) || !(s.flags & T3D_AUG_ROTATE)) return;
  const bool w2 = e->flags & T3D_CHAIN_WARP2;
  if (second && !w2) return;
  const bool last = second || !w2;
  t3d_aug_sample ws;                             // the previous pass's image as an arena slot, warped by aug_pixel
  ws.offset = (long long)i * plane * 3, ws.h = oh, ws.w = ow;
  ws.flags = T3D_AUG_ROTATE | (last ? s.flags & T3D_AUG_SWAP_RB : 0);
  ws.alpha = 1.f, ws.beta255 = 0.f, ws.reserved = 0;
#pragma unroll
  for (int k = 0; k < 6; ++k) ws.m[k] = second ? e->m2[k] : s.m[k];
  const long long bytes = (long long)B * plane * 3;
  unsigned char* dst = (last ? out : to) + (long long)i * plane * 3;
  const int nrun = (plane + AUG_PIX - 1) / AUG_PIX;
  for (int t = blockIdx.x * 256 + threadIdx.x; t < nrun; t += gridDim.x * 256) {
    const int r0 = t * AUG_PIX, n = min(AUG_PIX, plane - r0);
    unsigned int word[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < AUG_PIX; ++k) {
      if (k >= n) break;
      const int r = r0 + k;
      int px[3];
      aug_pixel<ArenaSrc>(from, bytes, ws, r % ow, r / ow, oh, ow, px);
      pack_px(word, k, px, false);
    }
    store_run(dst, r0, n, word);
  }
}

template <class Src>
int chain_launch(const unsigned char* src, long long src_bytes, const void* samples, const void* chains, void* scratch,
                 long long scratch_bytes, unsigned char* out, int B, int oh, int ow, int stages, void* stream) {
  if (!src || !samples || !chains || !out || src_bytes <= 0 || B < 0 || B > 65535 || oh <= 0 || ow <= 0 ||
      (long long)oh * ow > (1 << 24) || (reinterpret_cast<uintptr_t>(out) & 3) ||
      (stages & ~(T3D_STAGE_MEAN | T3D_STAGE_WARP | T3D_STAGE_WARP2)) || ((stages & T3D_STAGE_WARP2) && !(stages & T3D_STAGE_WARP)))
    return T3D_ERR_ARG;
  const int nwarp = ((stages & T3D_STAGE_WARP) ? 1 : 0) + ((stages & T3D_STAGE_WARP2) ? 1 : 0);
  const long long image = ((long long)B * oh * ow * 3 + 7) / 8 * 8;
  if (!scratch || (reinterpret_cast<uintptr_t>(scratch) & 7) || scratch_bytes < 8ll * B + nwarp * image) return T3D_ERR_ARG;
  if (B == 0) return T3D_OK;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const t3d_aug_sample* sp = reinterpret_cast<const t3d_aug_sample*>(samples);
  const t3d_aug_chain* cp = reinterpret_cast<const t3d_aug_chain*>(chains);
  unsigned long long* sums = reinterpret_cast<unsigned long long*>(scratch);
  unsigned char* tmp_a = reinterpret_cast<unsigned char*>(scratch) + 8ll * B;      // the colour pass's image (first warp's source)
  unsigned char* tmp_b = tmp_a + image;                                            // the first warp's image (second warp's source)
  const int plane = oh * ow;
  const int nblk = (plane + AUG_PIX * 256 - 1) / (AUG_PIX * 256);
  const dim3 grid(nblk > 1024 ? 1024 : nblk, B);
  if (stages & T3D_STAGE_MEAN) {
    if (hipMemsetAsync(sums, 0, 8ll * B, st) != hipSuccess) return T3D_ERR_LAUNCH;
    T3D_LAUNCH(chain_mean_kernel<Src>, grid, dim3(256), 0, st, src, src_bytes, sp, cp, sums, oh, ow, stages);
  }
  T3D_LAUNCH(chain_colour_kernel<Src>, grid, dim3(256), 0, st, src, src_bytes, sp, cp, sums, tmp_a, out, oh, ow, stages);
  if (stages & T3D_STAGE_WARP)
    T3D_LAUNCH(chain_warp_kernel, grid, dim3(256), 0, st, sp, cp, tmp_a, tmp_b, out, B, oh, ow, stages, 0);
  if (stages & T3D_STAGE_WARP2)
    T3D_LAUNCH(chain_warp_kernel, grid, dim3(256), 0, st, sp, cp, tmp_b, tmp_b, out, B, oh, ow, stages, 1);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

}  // namespace

extern "C" int t3d_augment_chain_crops_u8(const unsigned char* src, long long src_bytes, const void* samples, const void* chains,
                                          void* scratch, long long scratch_bytes, unsigned char* out, int B, int oh, int ow,
                                          int stages, void* stream) {
  return chain_launch<CropSrc>(src, src_bytes, samples, chains, scratch, scratch_bytes, out, B, oh, ow, stages, stream);
}

extern "C" int t3d_augment_chain_resized_u8(const unsigned char* arena, long long arena_bytes, const void* samples,
                                            const void* chains, void* scratch, long long scratch_bytes, unsigned char* out, int B,
                                            int oh, int ow, int stages, void* stream) {
  return chain_launch<ArenaSrc>(arena, arena_bytes, samples, chains, scratch, scratch_bytes, out, B, oh, ow, stages, stream);
}
