// What ONE LANE of the device JPEG decode does (csrc/jpeg.hip launches it; include/t3d.h states the arithmetic): the checked
// per-image geometry, the bit reader, the decode of one segment, the inverse DCT of one block, one run of four output pixels;
// and the same for one pixel rectangle of an image (t3d_jpeg_decode_roi_u8), on a workspace that holds its MCU rectangle only.
// The segment parser exists once (decode_segment): an item is a window of its image (Roi), a whole frame is the item whose
// window is the image (whole), and RECT says at compile time whether MCUs outside the window exist.  The IDCT and the pixel
// arithmetic are shared as they always were.  The item checks (geom, roi_geom) and the four-pixel stores (colour_run,
// colour_run_roi) stay two each: shared forms of them were built and made whole-frame decodes slower (finding 71).
// Like csrc/jpeg_index.h it has no HIP include, so the very code the kernels run also compiles for the host, where
// tools/jpeg_index_check.cpp walks it (tests/test_jpeg_lane_host.py; under the address and undefined-behaviour sanitizers by hand).
#pragma once
#include "jpeg_index.h"

#ifdef __HIPCC__
#define T3D_JPEG_LANE __device__ __forceinline__
#else
#define T3D_JPEG_LANE inline
#endif

namespace t3d_jpeg_lane {

template <class T> T3D_JPEG_LANE T lo(T a, T b) { return a < b ? a : b; }
template <class T> T3D_JPEG_LANE T hi(T a, T b) { return a > b ? a : b; }
T3D_JPEG_LANE int clamp255(int v) { return lo(hi(v, 0), 255); }
struct alignas(16) Int4 { int x, y, z, w; };
struct alignas(8) UInt2 { unsigned int x, y; };

// What the kernels need of one image, or ok == false.  Every field is checked here, by every kernel, before it is used.
struct Geom {
  bool ok;
  int h, w, ncomp, sampling, mcus_x, mcus_y, nmcu, seg_mcus, nseg, bpm;      // bpm: blocks per MCU
  long long nblocks;
  const unsigned char* scan;
  long long scan_bytes;
  const t3d_jpeg_seg* segs;
  unsigned char* out;
  short* coef;                   // [nblocks][64]
  unsigned char* planes;         // [nblocks][64]: the component planes, raster, one behind the other
};

T3D_JPEG_LANE Geom geom(const unsigned char* data, long long data_bytes, const t3d_jpeg_info* info, const t3d_jpeg_seg* segs,
                        long long total_segs, const t3d_jpeg_item& it, unsigned char* out, long long out_bytes, void* work,
                        long long total_blocks) {
  Geom g;
  g.ok = false;
  g.h = info->h, g.w = info->w, g.ncomp = info->ncomp, g.sampling = info->sampling;
  g.mcus_x = info->mcus_x, g.mcus_y = info->mcus_y, g.seg_mcus = info->seg_mcus, g.nseg = info->nseg;
  g.nmcu = g.bpm = 0, g.nblocks = 0, g.scan = nullptr, g.scan_bytes = 0, g.segs = nullptr, g.out = nullptr, g.coef = nullptr;
  g.planes = nullptr;
  if (g.h < 1 || g.w < 1 || g.h > 65535 || g.w > 65535) return g;
  if (g.sampling != T3D_JPEG_GRAY && g.sampling != T3D_JPEG_444 && g.sampling != T3D_JPEG_420) return g;
  if (g.ncomp != (g.sampling == T3D_JPEG_GRAY ? 1 : 3)) return g;
  const int px = g.sampling == T3D_JPEG_420 ? 16 : 8;
  if (g.mcus_x != (g.w + px - 1) / px || g.mcus_y != (g.h + px - 1) / px) return g;
  g.nmcu = g.mcus_x * g.mcus_y;                                             // <= 8192 * 8192
  if (g.seg_mcus < 1 || g.nseg != (int)(((long long)g.nmcu + g.seg_mcus - 1) / g.seg_mcus)) return g;
  g.bpm = t3d_jpeg_mcu_blocks(g.sampling);
  g.nblocks = (long long)g.nmcu * g.bpm;
  for (int c = 0; c < g.ncomp; ++c)
    if (info->comp_dc[c] > 1 || info->comp_ac[c] > 1) return g;
  const long long so = info->scan_offset, sb = info->scan_bytes;
  if (it.file_offset < 0 || it.file_bytes < 0 || it.file_offset > data_bytes || it.file_bytes > data_bytes - it.file_offset) return g;
  if (so < 0 || sb < 0 || so > it.file_bytes || sb > it.file_bytes - so || sb > 0xFFFFFFFFll) return g;
  if (it.seg_offset < 0 || it.seg_offset > total_segs || g.nseg > total_segs - it.seg_offset) return g;
  const long long ob = (long long)g.h * g.w * 3;
  if (it.out_offset < 0 || it.out_offset > out_bytes || ob > out_bytes - it.out_offset) return g;
  if (it.block_offset < 0 || it.block_offset > total_blocks || g.nblocks > total_blocks - it.block_offset) return g;
  g.scan = data + it.file_offset + so;
  g.scan_bytes = sb;
  g.segs = segs + it.seg_offset;
  g.out = out + it.out_offset;
  g.coef = reinterpret_cast<short*>(work) + it.block_offset * 64;
  g.planes = reinterpret_cast<unsigned char*>(work) + total_blocks * 128 + it.block_offset * 64;
  g.ok = true;
  return g;
}

// component c of the image: the first of its blocks (its plane starts 64 bytes a block into `planes`) and its size in blocks
struct Plane { long long first; int bw, bh; };
T3D_JPEG_LANE Plane plane(const Geom& g, int c) {
  Plane p;
  const int f = g.sampling == T3D_JPEG_420 ? 2 : 1;
  const long long luma = (long long)g.nmcu * f * f;
  p.bw = g.mcus_x * (c == 0 ? f : 1), p.bh = g.mcus_y * (c == 0 ? f : 1);
  p.first = c == 0 ? 0 : luma + (long long)(c - 1) * g.nmcu;
  return p;
}

// ---- entropy ---------------------------------------------------------------------------------------------------------------
// The scan from byte `pos` on: a 64-bit window (valid bits at its low end), refilled when 32 bits or fewer are left with up to
// four stream bytes that were loaded together.  FF 00 is one data byte FF; FF + anything else, or the scan's end, stops the
// reader for good: from there it feeds zero bits and does not advance.
// Of the scan, p holds the n bytes from byte `first` on (the whole scan: first 0); a byte outside them reads as a marker.
struct Bits {
  const unsigned char* p;
  unsigned int n, pos, first;
  unsigned long long buf;
  int cnt;
  bool stopped;

  T3D_JPEG_LANE unsigned int at(unsigned long long i) const {      // (behind the scan, or in front of `first`: a marker)
    i -= first;                                         // (wraps for i < first: not below n)
    return i < n ? p[i] : 0xFFu;
  }
  T3D_JPEG_LANE void refill() {
    while (cnt <= 32) {
      if (stopped) {
        buf <<= 32;
        cnt += 32;
        break;
      }
      unsigned int b[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) b[i] = at((unsigned long long)pos + i);
      int used = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (used > i || stopped) continue;              // a stuffed 00 that went with its FF
        if (b[i] == 0xFFu) {
          if (b[i + 1] != 0u) {
            stopped = true;
            continue;
          }
          used = i + 2;
        } else {
          used = i + 1;
        }
        buf = (buf << 8) | b[i];
        cnt += 8;
      }
      pos += used;
    }
  }
  T3D_JPEG_LANE unsigned int peek16() const { return (unsigned int)(buf >> (cnt - 16)) & 0xFFFFu; }    // cnt >= 16
  T3D_JPEG_LANE int get(int k) {                        // k <= 16 <= cnt
    cnt -= k;
    return (int)((unsigned int)(buf >> cnt) & ((1u << k) - 1u));
  }
};

// ---- inverse DCT -----------------------------------------------------------------------------------------------------------
// jpeg_idct_islow's butterfly on eight values; SHIFT: 11 (columns) or 18 (rows).  Unsigned arithmetic where a stream that no
// encoder makes could overflow (it wraps, as the int32 definition says); the shifts are arithmetic.
template <int SHIFT>
T3D_JPEG_LANE void idct8(const int in[8], int o[8]) {
  typedef unsigned int U;
  U z2 = (U)in[2], z3 = (U)in[6];
  U z1 = (z2 + z3) * 4433u;
  U tmp2 = z1 - z3 * 15137u;
  U tmp3 = z1 + z2 * 6270u;
  z2 = (U)in[0], z3 = (U)in[4];
  U tmp0 = (z2 + z3) << 13;
  U tmp1 = (z2 - z3) << 13;
  const U tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
  tmp0 = (U)in[7], tmp1 = (U)in[5], tmp2 = (U)in[3], tmp3 = (U)in[1];
  z1 = tmp0 + tmp3, z2 = tmp1 + tmp2, z3 = tmp0 + tmp2;
  U z4 = tmp1 + tmp3;
  const U z5 = (z3 + z4) * 9633u;
  tmp0 *= 2446u, tmp1 *= 16819u, tmp2 *= 25172u, tmp3 *= 12299u;
  z1 *= (U)-7373, z2 *= (U)-20995, z3 *= (U)-16069, z4 *= (U)-3196;
  z3 += z5, z4 += z5;
  tmp0 += z1 + z3, tmp1 += z2 + z4, tmp2 += z2 + z3, tmp3 += z1 + z4;
  const U rnd = 1u << (SHIFT - 1);
  o[0] = (int)(tmp10 + tmp3 + rnd) >> SHIFT;
  o[7] = (int)(tmp10 - tmp3 + rnd) >> SHIFT;
  o[1] = (int)(tmp11 + tmp2 + rnd) >> SHIFT;
  o[6] = (int)(tmp11 - tmp2 + rnd) >> SHIFT;
  o[2] = (int)(tmp12 + tmp1 + rnd) >> SHIFT;
  o[5] = (int)(tmp12 - tmp1 + rnd) >> SHIFT;
  o[3] = (int)(tmp13 + tmp0 + rnd) >> SHIFT;
  o[4] = (int)(tmp13 - tmp0 + rnd) >> SHIFT;
}

// block blk of a checked image: dequantise (quant [3][64], natural order), both passes, 8 x 8 samples into its plane
T3D_JPEG_LANE void idct_block(const Geom& g, const int* quant, long long blk) {
  const Plane pl1 = plane(g, 1), pl2 = plane(g, 2);
  const int c = blk < pl1.first || g.ncomp == 1 ? 0 : (blk < pl2.first ? 1 : 2);
  const Plane pl = c == 0 ? plane(g, 0) : (c == 1 ? pl1 : pl2);
  const int rel = (int)(blk - pl.first), by = rel / pl.bw, bx = rel - by * pl.bw;
  const short* src = g.coef + blk * 64;
  const int* q = quant + 64 * c;
  int ws[64];
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    const Int4 v = *reinterpret_cast<const Int4*>(src + 8 * r);             // (work is 16-byte aligned, a block 128 bytes)
    const int pair[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ws[8 * r + 2 * j] = (int)(short)(pair[j] & 0xFFFF) * q[8 * r + 2 * j];
      ws[8 * r + 2 * j + 1] = (pair[j] >> 16) * q[8 * r + 2 * j + 1];
    }
  }
#pragma unroll
  for (int x = 0; x < 8; ++x) {                         // columns
    int in[8], o[8];
#pragma unroll
    for (int y = 0; y < 8; ++y) in[y] = ws[8 * y + x];
    idct8<11>(in, o);
#pragma unroll
    for (int y = 0; y < 8; ++y) ws[8 * y + x] = o[y];
  }
  const long long stride = (long long)pl.bw * 8;
  unsigned char* dst = g.planes + pl.first * 64 + (long long)by * 8 * stride + bx * 8;      // 8-byte aligned
#pragma unroll
  for (int y = 0; y < 8; ++y) {                         // rows
    int o[8];
    idct8<18>(ws + 8 * y, o);
    UInt2 w;
    w.x = w.y = 0;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      w.x |= (unsigned int)clamp255(o[x] + 128) << (8 * x);
      w.y |= (unsigned int)clamp255(o[x + 4] + 128) << (8 * x);
    }
    *reinterpret_cast<UInt2*>(dst + y * stride) = w;
  }
}

// ---- chroma upsampling and colour ------------------------------------------------------------------------------------------
// one chroma sample of pixel (y, x) of a 4:2:0 image: s the plane (stride bytes a row) from chroma sample (oy, ox) of the image
// on, dh x dw real samples in the whole image
T3D_JPEG_LANE int up420(const unsigned char* s, long long stride, int dh, int dw, int y, int x, int oy, int ox) {
  const int r = y >> 1, cx = x >> 1, k = cx - ox;
  if (dw <= 2) return s[(r - oy) * stride + k];
  const int r2 = (y & 1) ? lo(r + 1, dh - 1) : hi(r - 1, 0);
  const unsigned char* a = s + (r - oy) * stride;
  const unsigned char* b = s + (r2 - oy) * stride;
  const int here = 3 * a[k] + b[k];
  if (x & 1) {
    if (cx == dw - 1) return (4 * here + 7) >> 4;
    return (3 * here + 3 * a[k + 1] + b[k + 1] + 7) >> 4;
  }
  if (cx == 0) return (4 * here + 8) >> 4;
  return (3 * here + 3 * a[k - 1] + b[k - 1] + 8) >> 4;
}

// pixel (y, x) of a checked image -> R, G, B; the planes begin at luma sample (oy, ox) of the image (multiples of the MCU)
T3D_JPEG_LANE void pixel_at(const Geom& g, int y, int x, int oy, int ox, int px[3]) {
  const Plane pl0 = plane(g, 0), pl1 = plane(g, 1), pl2 = plane(g, 2);
  const long long ystride = (long long)pl0.bw * 8, cstride = (long long)pl1.bw * 8;
  const int Y = g.planes[(y - oy) * ystride + (x - ox)];
  if (g.ncomp == 1) {
    px[0] = px[1] = px[2] = Y;
    return;
  }
  const unsigned char* pcb = g.planes + pl1.first * 64;
  const unsigned char* pcr = g.planes + pl2.first * 64;
  int cb, cr;
  if (g.sampling == T3D_JPEG_420) {
    const int dh = (g.h + 1) >> 1, dw = (g.w + 1) >> 1;
    cb = up420(pcb, cstride, dh, dw, y, x, oy >> 1, ox >> 1);
    cr = up420(pcr, cstride, dh, dw, y, x, oy >> 1, ox >> 1);
  } else {
    cb = pcb[(y - oy) * cstride + (x - ox)];
    cr = pcr[(y - oy) * cstride + (x - ox)];
  }
  cb -= 128, cr -= 128;
  px[0] = clamp255(Y + ((91881 * cr + 32768) >> 16));
  px[1] = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
  px[2] = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

T3D_JPEG_LANE void pixel(const Geom& g, int y, int x, int px[3]) { pixel_at(g, y, x, 0, 0, px); }

// run t of a checked image: its pixels 4t .. 4t + 3, as three dwords where the image is dword aligned and the run whole
T3D_JPEG_LANE void colour_run(const Geom& g, long long t, bool aligned) {
  const long long npix = (long long)g.h * g.w, r0 = 4 * t;
  // (h, w <= 65535: a pixel index fits 32 bits unsigned -- one 32-bit division a run, then steps)
  int y = (int)((unsigned int)r0 / (unsigned int)g.w), x = (int)((unsigned int)r0 - (unsigned int)y * (unsigned int)g.w);
  if (aligned && r0 + 4 <= npix) {
    unsigned int word[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int px[3];
      pixel(g, y, x, px);
      if (++x == g.w) x = 0, ++y;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int b = 3 * k + c;
        word[b >> 2] |= (unsigned int)px[c] << (8 * (b & 3));
      }
    }
    unsigned int* o4 = reinterpret_cast<unsigned int*>(g.out + 3 * r0);
    o4[0] = word[0], o4[1] = word[1], o4[2] = word[2];
  } else {
    for (long long r = r0; r < lo(r0 + 4, npix); ++r) {
      int px[3];
      pixel(g, y, x, px);
      if (++x == g.w) x = 0, ++y;
      g.out[3 * r] = (unsigned char)px[0], g.out[3 * r + 1] = (unsigned char)px[1], g.out[3 * r + 2] = (unsigned char)px[2];
    }
  }
}

// ---- a pixel rectangle of an image (t3d_jpeg_decode_roi_u8) ------------------------------------------------------------------
// The MCUs the decode above reads for the pixels [x0, x1) x [y0, y1) of an h x w image (0 <= x0 < x1 <= w, 0 <= y0 < y1 <= h).
// Gray and 4:4:4: the MCUs of the pixels.  4:2:0, dw > 2: pixel (y, x) reads chroma rows y >> 1 and (y >> 1) - 1 (y even) or + 1
// (y odd), columns x >> 1 and (x >> 1) - 1 (x even) or + 1 (x odd), clamped to the dh x dw real samples -- the rectangle halved
// and dilated by the one sample its edge pixels reach for; chroma sample s lies in MCU s >> 3, which holds the luma too.
struct McuRect { int mx0, my0, mx1, my1; };
T3D_JPEG_LANE McuRect roi_mcus(int sampling, int h, int w, int x0, int y0, int x1, int y1) {
  McuRect r;
  if (sampling != T3D_JPEG_420) {
    r.mx0 = x0 >> 3, r.my0 = y0 >> 3, r.mx1 = ((x1 - 1) >> 3) + 1, r.my1 = ((y1 - 1) >> 3) + 1;
    return r;
  }
  const int dh = (h + 1) >> 1, dw = (w + 1) >> 1;
  int cx0 = x0 >> 1, cx1 = (x1 - 1) >> 1, cy0 = y0 >> 1, cy1 = (y1 - 1) >> 1;      // chroma samples, inclusive
  if (dw > 2) {
    if (!(x0 & 1)) cx0 = hi(cx0 - 1, 0);
    if ((x1 - 1) & 1) cx1 = lo(cx1 + 1, dw - 1);
    if (!(y0 & 1)) cy0 = hi(cy0 - 1, 0);
    if ((y1 - 1) & 1) cy1 = lo(cy1 + 1, dh - 1);
  }
  r.mx0 = cx0 >> 3, r.my0 = cy0 >> 3, r.mx1 = (cx1 >> 3) + 1, r.my1 = (cy1 >> 3) + 1;
  return r;
}

// One item of t3d_jpeg_decode_roi_u8, or g.ok == false.  g is the geometry the lane functions above take, made COMPACT: h, w,
// sampling, seg_mcus, nseg, bpm are the image's; mcus_x, mcus_y, nmcu, nblocks, coef, planes are those of the MCU rectangle
// [mx0, mx1) x [my0, my1), whose blocks are all the workspace holds; scan points at the uploaded bytes, which are the scan's
// [span_first, span_first + span_bytes); segs[k] is the image's segment seg_first + k.
struct Roi {
  Geom g;
  int x0, y0, x1, y1, mx0, my0, mx1, my1;
  int img_mcus_x, img_nmcu;
  long long span_first, span_bytes;
  int seg_first, seg_count;
  int per_row;                   // entropy lanes per MCU row of the rectangle (roi_lane_segment)
};

// rect: x0 y0 x1 y1 mx0 my0 mx1 my1 seg_first seg_count (+ 2 reserved) of include/t3d.h
T3D_JPEG_LANE Roi roi_geom(const unsigned char* data, long long data_bytes, const t3d_jpeg_info* info, const t3d_jpeg_seg* segs,
                           long long total_segs, const t3d_jpeg_item& it, const int* rect, unsigned char* out, long long out_bytes,
                           void* work, long long total_blocks) {
  Roi r;
  Geom& g = r.g;
  g.ok = false;
  g.h = info->h, g.w = info->w, g.ncomp = info->ncomp, g.sampling = info->sampling;
  g.seg_mcus = info->seg_mcus, g.nseg = info->nseg;
  g.mcus_x = g.mcus_y = g.nmcu = g.bpm = 0, g.nblocks = 0, g.scan = nullptr, g.scan_bytes = 0, g.segs = nullptr, g.out = nullptr;
  g.coef = nullptr, g.planes = nullptr;
  r.x0 = rect[0], r.y0 = rect[1], r.x1 = rect[2], r.y1 = rect[3], r.mx0 = rect[4], r.my0 = rect[5], r.mx1 = rect[6], r.my1 = rect[7];
  r.seg_first = rect[8], r.seg_count = rect[9];
  r.img_mcus_x = info->mcus_x, r.img_nmcu = 0, r.span_first = it.reserved, r.span_bytes = it.file_bytes, r.per_row = 0;
  if (g.h < 1 || g.w < 1 || g.h > 65535 || g.w > 65535) return r;
  if (g.sampling != T3D_JPEG_GRAY && g.sampling != T3D_JPEG_444 && g.sampling != T3D_JPEG_420) return r;
  if (g.ncomp != (g.sampling == T3D_JPEG_GRAY ? 1 : 3)) return r;
  const int px = g.sampling == T3D_JPEG_420 ? 16 : 8;
  if (info->mcus_x != (g.w + px - 1) / px || info->mcus_y != (g.h + px - 1) / px) return r;
  r.img_nmcu = info->mcus_x * info->mcus_y;                                   // <= 8192 * 8192
  if (g.seg_mcus < 1 || g.nseg != (int)(((long long)r.img_nmcu + g.seg_mcus - 1) / g.seg_mcus)) return r;
  for (int c = 0; c < g.ncomp; ++c)
    if (info->comp_dc[c] > 1 || info->comp_ac[c] > 1) return r;
  // the pixel rectangle, and an MCU rectangle that holds every block its pixels read
  if (r.x0 < 0 || r.y0 < 0 || r.x0 >= r.x1 || r.y0 >= r.y1 || r.x1 > g.w || r.y1 > g.h) return r;
  if (r.mx0 < 0 || r.my0 < 0 || r.mx0 >= r.mx1 || r.my0 >= r.my1 || r.mx1 > info->mcus_x || r.my1 > info->mcus_y) return r;
  const McuRect need = roi_mcus(g.sampling, g.h, g.w, r.x0, r.y0, r.x1, r.y1);
  if (r.mx0 > need.mx0 || r.my0 > need.my0 || r.mx1 < need.mx1 || r.my1 < need.my1) return r;
  // the uploaded bytes within data and within the scan
  const long long sb = info->scan_bytes;
  if (sb < 0 || sb > 0xFFFFFFFFll) return r;
  if (it.file_offset < 0 || it.file_bytes < 0 || it.file_offset > data_bytes || it.file_bytes > data_bytes - it.file_offset) return r;
  if (r.span_first < 0 || r.span_first > sb || r.span_bytes > sb - r.span_first) return r;
  // the uploaded segments hold the first and the last one the rectangle needs
  const int rw = r.mx1 - r.mx0, rh = r.my1 - r.my0;
  const int s_lo = (r.my0 * r.img_mcus_x + r.mx0) / g.seg_mcus, s_hi = ((r.my1 - 1) * r.img_mcus_x + r.mx1 - 1) / g.seg_mcus;
  if (r.seg_first < 0 || r.seg_count < 1 || r.seg_count > g.nseg - r.seg_first) return r;
  if (s_lo < r.seg_first || s_hi - r.seg_first >= r.seg_count) return r;
  if (it.seg_offset < 0 || it.seg_offset > total_segs || r.seg_count > total_segs - it.seg_offset) return r;
  const long long ob = (long long)(r.y1 - r.y0) * (r.x1 - r.x0) * 3;
  if (it.out_offset < 0 || it.out_offset > out_bytes || ob > out_bytes - it.out_offset) return r;
  g.bpm = t3d_jpeg_mcu_blocks(g.sampling);
  g.mcus_x = rw, g.mcus_y = rh, g.nmcu = rw * rh;
  g.nblocks = (long long)g.nmcu * g.bpm;
  if (it.block_offset < 0 || it.block_offset > total_blocks || g.nblocks > total_blocks - it.block_offset) return r;
  r.per_row = (rw - 1) / g.seg_mcus + 2;
  g.scan = data + it.file_offset;
  g.scan_bytes = sb;
  g.segs = segs + it.seg_offset;
  g.out = out + it.out_offset;
  g.coef = reinterpret_cast<short*>(work) + it.block_offset * 64;
  g.planes = reinterpret_cast<unsigned char*>(work) + total_blocks * 128 + it.block_offset * 64;
  g.ok = true;
  return r;
}

// geom's result as the item whose window is the image: every pixel, every MCU, every segment, the whole scan.  Only copies, so
// it may be made before g.ok is looked at (r.g.ok says the same); per_row 0: a whole frame has no lane map, a lane per segment.
T3D_JPEG_LANE Roi whole(const Geom& g) {
  Roi r;
  r.g = g;
  r.x0 = r.y0 = r.mx0 = r.my0 = r.seg_first = r.per_row = 0;
  r.x1 = g.w, r.y1 = g.h, r.mx1 = r.img_mcus_x = g.mcus_x, r.my1 = g.mcus_y, r.img_nmcu = g.nmcu, r.seg_count = g.nseg;
  r.span_first = 0, r.span_bytes = g.scan_bytes;
  return r;
}

// Entropy lane t of a checked rectangle item (t < rows * per_row) -> the segment it decodes, or -1.  The rectangle's MCU row `my`
// needs the segments of its MCUs my * mcus_x + mx0 .. + mx1 - 1, at most per_row of them; one that the row above already needed (a
// segment may straddle rows) is left to that row's lanes, so every needed segment comes up exactly once.
T3D_JPEG_LANE int roi_lane_segment(const Roi& r, long long t) {
  const int row = (int)(t / r.per_row), j = (int)(t - (long long)row * r.per_row);
  if (row >= r.my1 - r.my0) return -1;
  const int base = (r.my0 + row) * r.img_mcus_x, S = r.g.seg_mcus;
  int a = (base + r.mx0) / S;
  const int b = (base + r.mx1 - 1) / S;
  if (row > 0) a = hi(a, (base - r.img_mcus_x + r.mx1 - 1) / S + 1);
  return a + j <= b ? a + j : -1;
}

constexpr unsigned char zigzag[64] = T3D_JPEG_ZIGZAG;

// Segment s of a checked item (s < nseg; RECT: one roi_lane_segment gave): its MCUs [s * seg_mcus, ...) of the image parsed from
// the indexed position -- bits and DC predictors advance --, the non-zero quantised coefficients of those inside the window
// stored in natural order into their own (zeroed) blocks of the workspace.  tab: DC 0, DC 1, AC 0, AC 1.
// RECT false: the window is the image (geom), so every MCU is stored, at its image position; true: the parse ends behind the
// window's last MCU.  (A compile-time choice: the whole-frame lanes do not pay for the window test.)
// -> false: a code that does not exist (or a run past the block); the rest of the segment's blocks stay zero.
template <bool RECT>
T3D_JPEG_LANE bool decode_segment(const Roi& r, const t3d_jpeg_huff* tab, const int dci[3], const int aci[3], int s) {
  const Geom& g = r.g;
  const t3d_jpeg_seg sg = g.segs[s - r.seg_first];      // (roi_geom: the needed segments are among the uploaded ones)
  if (sg.byte < r.span_first || sg.byte - r.span_first >= r.span_bytes || sg.bit > 7) return false;
  Bits br;
  br.p = g.scan, br.n = (unsigned int)r.span_bytes, br.pos = sg.byte, br.first = (unsigned int)r.span_first, br.buf = 0, br.cnt = 0;
  br.stopped = false;
  br.refill();
  br.cnt -= sg.bit;                                     // (the first refill took at least one byte, or stopped and made 32 bits)
  int pred[3] = {sg.pred[0], sg.pred[1], sg.pred[2]};
  const int ybl = g.sampling == T3D_JPEG_420 ? 4 : 1;   // luma blocks of an MCU
  const long long first1 = plane(g, 1).first, first2 = plane(g, 2).first;
  const int last = (r.my1 - 1) * r.img_mcus_x + r.mx1 - 1;                     // the window's last MCU
  const int m0 = s * g.seg_mcus, end = r.img_nmcu - m0 > g.seg_mcus ? m0 + g.seg_mcus : r.img_nmcu;      // m0 < nmcu <= 2^26
  const int m1 = RECT ? lo(end, last + 1) : end;
  for (int m = m0; m < m1; ++m) {
    const int my = m / r.img_mcus_x, mx = m - my * r.img_mcus_x;
    const bool in = RECT ? mx >= r.mx0 && mx < r.mx1 && my >= r.my0 && my < r.my1 : true;
    const int cy = RECT ? my - r.my0 : my, cx = RECT ? mx - r.mx0 : mx, cm = RECT ? cy * g.mcus_x + cx : m;      // within the window
    for (int b = 0; b < g.bpm; ++b) {
      const int c = b < ybl ? 0 : b - ybl + 1;
      long long blk;
      if (c == 0) blk = ybl == 4 ? (long long)(2 * cy + (b >> 1)) * (2 * g.mcus_x) + 2 * cx + (b & 1) : (long long)cm;
      else blk = (c == 1 ? first1 : first2) + cm;
      short* dst = g.coef + (in ? blk : 0) * 64;        // in: blk < nblocks, one of this MCU's own blocks; else: not written
      const t3d_jpeg_huff* hd = tab + dci[c];
      const t3d_jpeg_huff* ha = tab + aci[c];
      br.refill();
      int e = t3d_jpeg_huff_decode(hd, br.peek16());
      if (e < 0 || (e & 255) > 15) return false;
      br.cnt -= e >> 8;
      const int t = e & 255;
      pred[c] = (int)((unsigned int)pred[c] + (unsigned int)t3d_jpeg_extend(br.get(t), t));      // (wraps; never overflows)
      if (in && pred[c] != 0) dst[0] = (short)pred[c];
      for (int k = 1; k < 64;) {                        // k grows by at least 1 a round
        br.refill();
        e = t3d_jpeg_huff_decode(ha, br.peek16());
        if (e < 0) return false;
        br.cnt -= e >> 8;
        const int rr = (e >> 4) & 15, sz = e & 15;
        if (sz == 0) {
          if (rr != 15) break;
          k += 16;
          if (k > 64) return false;
          continue;
        }
        k += rr;
        if (k > 63) return false;
        const int v = t3d_jpeg_extend(br.get(sz), sz);
        if (in) dst[zigzag[k]] = (short)v;
        ++k;
      }
    }
  }
  return true;
}

// run t of a checked item: up to four consecutive pixels of one row of the rectangle (runs do not wrap), as three dwords where
// the run is whole and its address dword aligned (a crop's offset and width are arbitrary: every lane looks at its own address)
T3D_JPEG_LANE void colour_run_roi(const Roi& r, long long t) {
  const int rw = r.x1 - r.x0, rpr = (rw + 3) >> 2;
  const int row = (int)(t / rpr), xr = (int)(t - (long long)row * rpr) * 4, n = lo(4, rw - xr);
  const int y = r.y0 + row, x = r.x0 + xr;
  const int px_mcu = r.g.sampling == T3D_JPEG_420 ? 16 : 8, oy = r.my0 * px_mcu, ox = r.mx0 * px_mcu;
  unsigned char* o = r.g.out + ((long long)row * rw + xr) * 3;
  if (n == 4 && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    unsigned int word[3] = {0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      int px[3];
      pixel_at(r.g, y, x + k, oy, ox, px);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int b = 3 * k + c;
        word[b >> 2] |= (unsigned int)px[c] << (8 * (b & 3));
      }
    }
    unsigned int* o4 = reinterpret_cast<unsigned int*>(o);
    o4[0] = word[0], o4[1] = word[1], o4[2] = word[2];
  } else {
    for (int k = 0; k < n; ++k) {
      int px[3];
      pixel_at(r.g, y, x + k, oy, ox, px);
      o[3 * k] = (unsigned char)px[0], o[3 * k + 1] = (unsigned char)px[1], o[3 * k + 2] = (unsigned char)px[2];
    }
  }
}

}  // namespace t3d_jpeg_lane
