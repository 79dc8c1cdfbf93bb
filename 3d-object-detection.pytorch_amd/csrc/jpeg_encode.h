// The device JPEG encoder (include/t3d.h next to t3d_jpeg_encode_setup states the arithmetic; csrc/jpeg_encode.hip launches it):
// the host-only table setup, the layout of a call's work buffer, and what ONE LANE of every kernel does -- the transform of one
// 8x8 block, the walk of one segment (counting or emitting its codes), the FF count and the scatter of one 64-byte chunk.
// Like csrc/jpeg_decode.h it has no HIP include, so the very code the kernels run also compiles for the host, where
// tools/jpeg_encode_check.cpp runs it lane by lane (under the address and undefined-behaviour sanitizers).
#pragma once
#include <initializer_list>

#include "jpeg_index.h"

#ifdef __HIPCC__
#define T3D_ENC_LANE __device__ __forceinline__
#define T3D_ENC_OR(p, v) atomicOr((p), (v))
#else
#define T3D_ENC_LANE inline
#define T3D_ENC_OR(p, v) (*(p) |= (v))
#endif

namespace t3d_jpeg_enc {

constexpr int kHeaderBytes = 623;
constexpr int kChunk = 64;               // bytes of the unstuffed stream per stuffing lane

// ---- t3d_jpeg_encode_setup: host only ---------------------------------------------------------------------------------------
namespace annex_k {
constexpr unsigned char luma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57,
                                    69, 56, 14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64,
                                    81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char chroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                      99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                      99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr unsigned char dc_bits[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
constexpr unsigned char ac_bits[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77}};
constexpr unsigned char ac_vals[2][162] = {
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa}};
}  // namespace annex_k

// the MCU grid of an h x w frame: what setup writes and every entry point checks a caller's struct against
struct Grid { int mcus_x, mcus_y, bpm, blocks, luma_rows, luma_cols; };
inline bool grid_of(int h, int w, int sampling, Grid* g) {
  if (h < 1 || w < 1 || h > 65535 || w > 65535 || (sampling != T3D_JPEG_444 && sampling != T3D_JPEG_420)) return false;
  const int px = sampling == T3D_JPEG_420 ? 16 : 8;
  g->mcus_x = (w + px - 1) / px, g->mcus_y = (h + px - 1) / px, g->bpm = sampling == T3D_JPEG_420 ? 6 : 3;
  g->blocks = g->mcus_x * g->mcus_y * g->bpm;           // <= 8192 * 8192 * 3
  g->luma_rows = (h + 7) / 8, g->luma_cols = (w + 7) / 8;
  return true;
}

// one DHT table (bits[16], n symbols) -> out[256] by symbol: length << 16 | code
inline void fill_codes(const unsigned char* bits, const unsigned char* vals, int n, unsigned int* out) {
  for (int i = 0; i < 256; ++i) out[i] = 0;
  unsigned int code = 0;
  int k = 0;
  for (int l = 1; l <= 16; ++l) {
    for (int j = 0; j < bits[l - 1] && k < n; ++j, ++k, ++code) out[vals[k]] = ((unsigned int)l << 16) | code;
    code <<= 1;
  }
}

inline int setup_impl(int h, int w, int quality, int sampling, t3d_jpeg_enc_tables* t) {
  Grid g;
  if (!t || quality < 1 || quality > 100 || !grid_of(h, w, sampling, &g)) return T3D_ERR_ARG;
  memset(t, 0, sizeof(*t));
  t->h = h, t->w = w, t->quality = quality, t->sampling = sampling;
  t->mcus_x = g.mcus_x, t->mcus_y = g.mcus_y, t->mcu_blocks = g.bpm, t->blocks = g.blocks;
  t->luma_rows = g.luma_rows, t->luma_cols = g.luma_cols;
  static const unsigned char zigzag[64] = T3D_JPEG_ZIGZAG;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  unsigned char q[2][64];
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 64; ++i) {
      int v = ((c ? annex_k::chroma[i] : annex_k::luma[i]) * scale + 50) / 100;
      v = v < 1 ? 1 : (v > 255 ? 255 : v);
      q[c][i] = (unsigned char)v;
      t->divisor[c][i] = (unsigned short)(8 * v);
    }
  unsigned char dc_vals[12];
  for (int i = 0; i < 12; ++i) dc_vals[i] = (unsigned char)i;
  for (int c = 0; c < 2; ++c) {
    fill_codes(annex_k::dc_bits[c], dc_vals, 12, t->huff[c]);
    fill_codes(annex_k::ac_bits[c], annex_k::ac_vals[c], 162, t->huff[2 + c]);
  }
  unsigned char* p = t->header;
  int n = 0;
  auto put = [&](std::initializer_list<int> b) { for (int v : b) p[n++] = (unsigned char)v; };
  put({0xFF, 0xD8, 0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0});
  for (int c = 0; c < 2; ++c) {
    put({0xFF, 0xDB, 0, 0x43, c});
    for (int k = 0; k < 64; ++k) p[n++] = q[c][zigzag[k]];
  }
  put({0xFF, 0xC0, 0, 0x11, 8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, sampling == T3D_JPEG_420 ? 0x22 : 0x11, 0, 2, 0x11, 1, 3, 0x11, 1});
  for (int i = 0; i < 4; ++i) {                         // DC 0, AC 0, DC 1, AC 1
    const int c = i >> 1, ac = i & 1, cnt = ac ? 162 : 12;
    put({0xFF, 0xC4, 0, 19 + cnt, (ac << 4) | c});
    for (int k = 0; k < 16; ++k) p[n++] = ac ? annex_k::ac_bits[c][k] : annex_k::dc_bits[c][k];
    for (int k = 0; k < cnt; ++k) p[n++] = ac ? annex_k::ac_vals[c][k] : dc_vals[k];
  }
  put({0xFF, 0xDA, 0, 12, 3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0});
  t->header_bytes = n;                                  // kHeaderBytes
  return n == kHeaderBytes ? T3D_OK : T3D_ERR_ARG;
}

// ---- one call: geometry and the work buffer ----------------------------------------------------------------------------------
// Everything the kernels index with, made on the host from checked arguments and passed to them by value.
// work: int16 coef [B][blocks][64] | uint64 seg [B][nseg + 1] (bit lengths, then exclusive bit offsets and the total) |
//       uint8 stream [B][ushare] (unstuffed, zeroed) | uint32 ff [B][nchunk + 1] (FF bytes per chunk, then their exclusive sums)
struct Geo {
  int h, w, sampling, mcus_x, mcus_y, nmcu, bpm, blocks, luma_rows, luma_cols, seg_mcus, nseg;
  long long cap, ushare, nchunk;         // a frame's slot in out; its share of the unstuffed stream (a multiple of kChunk); chunks of it
  long long off_seg, off_stream, off_ff, total;      // byte offsets within work
};

inline bool geo_of(int B, int h, int w, int sampling, int seg_mcus, long long cap_bytes, Geo* g) {
  Grid gr;
  if (B < 0 || B > 65535 || seg_mcus < 1 || cap_bytes < kHeaderBytes + 2 || cap_bytes > (1ll << 40) || !grid_of(h, w, sampling, &gr)) return false;
  g->h = h, g->w = w, g->sampling = sampling, g->mcus_x = gr.mcus_x, g->mcus_y = gr.mcus_y, g->nmcu = gr.mcus_x * gr.mcus_y;
  g->bpm = gr.bpm, g->blocks = gr.blocks, g->luma_rows = gr.luma_rows, g->luma_cols = gr.luma_cols, g->seg_mcus = seg_mcus;
  g->nseg = (int)(((long long)g->nmcu + seg_mcus - 1) / seg_mcus);
  g->cap = cap_bytes;
  g->ushare = (cap_bytes + kChunk - 1) / kChunk * kChunk;
  g->nchunk = g->ushare / kChunk;
  auto up16 = [](long long v) { return (v + 15) / 16 * 16; };
  g->off_seg = (long long)B * g->blocks * 128;
  g->off_stream = g->off_seg + up16((long long)B * (g->nseg + 1) * 8);
  g->off_ff = g->off_stream + (long long)B * g->ushare;
  g->total = g->off_ff + up16((long long)B * (g->nchunk + 1) * 4);
  return true;
}

// frame i's parts of the work buffer
T3D_ENC_LANE short* coef_of(const Geo& g, void* work, int i) { return reinterpret_cast<short*>(work) + (long long)i * g.blocks * 64; }
T3D_ENC_LANE unsigned long long* seg_of(const Geo& g, void* work, int i) {
  return reinterpret_cast<unsigned long long*>(reinterpret_cast<unsigned char*>(work) + g.off_seg) + (long long)i * (g.nseg + 1);
}
T3D_ENC_LANE unsigned int* stream_of(const Geo& g, void* work, int i) {
  return reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(work) + g.off_stream + (long long)i * g.ushare);
}
T3D_ENC_LANE unsigned int* ff_of(const Geo& g, void* work, int i) {
  return reinterpret_cast<unsigned int*>(reinterpret_cast<unsigned char*>(work) + g.off_ff) + (long long)i * (g.nchunk + 1);
}

struct alignas(16) Int4 { int x, y, z, w; };
template <class T> T3D_ENC_LANE T lo(T a, T b) { return a < b ? a : b; }
constexpr unsigned char zigzag[64] = T3D_JPEG_ZIGZAG;

// ---- transform ---------------------------------------------------------------------------------------------------------------
constexpr int fix16(double x) { return (int)(x * 65536 + 0.5); }
constexpr int fix13(double x) { return (int)(x * 8192 + 0.5); }

// component c of a pixel (jccolor)
template <int C> T3D_ENC_LANE int ycc(int r, int g, int b) {
  if (C == 0) return (fix16(.299) * r + fix16(.587) * g + fix16(.114) * b + 32768) >> 16;
  if (C == 1) return (-fix16(.16874) * r - fix16(.33126) * g + fix16(.5) * b + (128 << 16) + 32767) >> 16;
  return (fix16(.5) * r - fix16(.41869) * g - fix16(.08131) * b + (128 << 16) + 32767) >> 16;
}

// The N pixels of a frame row from column x0 (< w) on, columns beyond the image replicating the last one -> their 3N bytes as
// dwords (byte j: wds[j >> 2] >> 8 (j & 3)).  Dword loads where the run is whole and its address aligned (a 1080 x 1920
// frame's every run is), bytes otherwise.
template <int N> T3D_ENC_LANE void load_run(const unsigned char* row, int x0, int w, unsigned int* wds) {
  const unsigned char* p = row + 3 * (long long)x0;
  if (x0 + N <= w && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
#pragma unroll
    for (int i = 0; i < 3 * N / 4; ++i) wds[i] = reinterpret_cast<const unsigned int*>(p)[i];
  } else {
#pragma unroll
    for (int i = 0; i < 3 * N / 4; ++i) {
      unsigned int v = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int j = 4 * i + k, px = lo(x0 + j / 3, w - 1);
        v |= (unsigned int)row[3 * (long long)px + j % 3] << (8 * k);
      }
      wds[i] = v;
    }
  }
}
T3D_ENC_LANE int byte_of(const unsigned int* wds, int j) { return (int)((wds[j >> 2] >> (8 * (j & 3))) & 255u); }

// the 8 x 8 samples of block (by, bx) of component C at full resolution (Y; Cb, Cr of 4:4:4), rows and columns replicated
template <int C> T3D_ENC_LANE void samples_full(const Geo& g, const unsigned char* frame, int by, int bx, int* d) {
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const unsigned char* row = frame + (long long)lo(8 * by + y, g.h - 1) * g.w * 3;
    unsigned int wds[6];
    load_run<8>(row, 8 * bx, g.w, wds);
#pragma unroll
    for (int x = 0; x < 8; ++x) d[8 * y + x] = ycc<C>(byte_of(wds, 3 * x), byte_of(wds, 3 * x + 1), byte_of(wds, 3 * x + 2));
  }
}

// the 8 x 8 samples of chroma block (by, bx) of a 4:2:0 frame: h2v2 downsampling with the edge rules of the definition
template <int C> T3D_ENC_LANE void samples_420(const Geo& g, const unsigned char* frame, int by, int bx, int* d) {
  const int dh = (g.h + 1) >> 1;
#pragma unroll
  for (int y = 0; y < 8; ++y) {
    const int cy = lo(8 * by + y, dh - 1);              // the last DOWNSAMPLED row repeats
    int acc[8] = {1, 2, 1, 2, 1, 2, 1, 2};
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const unsigned char* row = frame + (long long)lo(2 * cy + v, g.h - 1) * g.w * 3;      // rows replicate to an even count
      unsigned int wds[12];
      load_run<16>(row, 16 * bx, g.w, wds);
#pragma unroll
      for (int x = 0; x < 16; ++x) acc[x >> 1] += ycc<C>(byte_of(wds, 3 * x), byte_of(wds, 3 * x + 1), byte_of(wds, 3 * x + 2));
    }
#pragma unroll
    for (int x = 0; x < 8; ++x) d[8 * y + x] = acc[x] >> 2;
  }
}

// jfdctint.c: one pass over eight values with stride S in d
template <bool FIRST, int S> T3D_ENC_LANE void fdct8(int* d) {
  constexpr int N = FIRST ? 11 : 15;
  const int t0 = d[0] + d[7 * S], t7 = d[0] - d[7 * S], t1 = d[S] + d[6 * S], t6 = d[S] - d[6 * S];
  const int t2 = d[2 * S] + d[5 * S], t5 = d[2 * S] - d[5 * S], t3 = d[3 * S] + d[4 * S], t4 = d[3 * S] - d[4 * S];
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  d[0] = FIRST ? (t10 + t11) * 4 : (t10 + t11 + 2) >> 2;
  d[4 * S] = FIRST ? (t10 - t11) * 4 : (t10 - t11 + 2) >> 2;
  int z1 = (t12 + t13) * fix13(0.541196100);
  d[2 * S] = (z1 + t13 * fix13(0.765366865) + (1 << (N - 1))) >> N;
  d[6 * S] = (z1 - t12 * fix13(1.847759065) + (1 << (N - 1))) >> N;
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
  const int z5 = (z3 + z4) * fix13(1.175875602);
  const int u4 = t4 * fix13(0.298631336), u5 = t5 * fix13(2.053119869), u6 = t6 * fix13(3.072711026), u7 = t7 * fix13(1.501321110);
  z1 *= -fix13(0.899976223), z2 *= -fix13(2.562915447);
  z3 = z3 * -fix13(1.961570560) + z5, z4 = z4 * -fix13(0.390180644) + z5;
  d[7 * S] = (u4 + z1 + z3 + (1 << (N - 1))) >> N;
  d[5 * S] = (u5 + z2 + z4 + (1 << (N - 1))) >> N;
  d[3 * S] = (u6 + z2 + z3 + (1 << (N - 1))) >> N;
  d[S] = (u7 + z1 + z4 + (1 << (N - 1))) >> N;
}

T3D_ENC_LANE int quantise(int c, int div) {
  const int a = c < 0 ? -c : c, q = (a + (div >> 1)) / div;
  return c < 0 ? -q : q;
}

// Lane t of a frame (t < g.blocks): one block, numbered plane by plane (all Y blocks in raster order, then Cb, then Cr) so
// that the lanes of a wave do the same work; its 64 quantised coefficients go to the block's place in SCAN order, zig-zag.
// divisor: [2][64], natural order.
T3D_ENC_LANE void transform_block(const Geo& g, const unsigned char* frame, const unsigned short* divisor, short* coef, int t) {
  const bool s420 = g.sampling == T3D_JPEG_420;
  const int ybl = s420 ? 4 : 1, ny = g.nmcu * ybl;
  int c, by, bx, pos;
  if (t < ny) {
    const int bw = g.mcus_x * (s420 ? 2 : 1);
    c = 0, by = t / bw, bx = t - by * bw;
    pos = s420 ? ((by >> 1) * g.mcus_x + (bx >> 1)) * 6 + (by & 1) * 2 + (bx & 1) : t * 3;
  } else {
    const int rel = t - ny;
    c = 1 + rel / g.nmcu;
    const int m = rel - (c - 1) * g.nmcu;
    by = m / g.mcus_x, bx = m - by * g.mcus_x;
    pos = m * g.bpm + ybl + c - 1;
  }
  Int4* dst = reinterpret_cast<Int4*>(coef + (long long)pos * 64);           // (work is 16-byte aligned, a block 128 bytes)
  int d[64];
  if (c == 0 && (by >= g.luma_rows || bx >= g.luma_cols)) {
    // a dummy block (4:2:0): the DC of the block before it in the MCU, which leads back to a REAL block of the MCU; a
    // block's unquantised DC is the sum of its samples - 64 * 128 (both FDCT passes are exact at output 0)
    int sy, sx;
    if (by >= g.luma_rows) sy = by - 1, sx = (bx | 1) < g.luma_cols ? (bx | 1) : (bx & ~1);
    else sy = by, sx = bx - 1;
    samples_full<0>(g, frame, sy, sx, d);
    int sum = -64 * 128;
#pragma unroll
    for (int i = 0; i < 64; ++i) sum += d[i];
    const Int4 zero = {0, 0, 0, 0};
    Int4 first = zero;
    first.x = quantise(sum, divisor[0]) & 0xFFFF;
    dst[0] = first;
#pragma unroll
    for (int i = 1; i < 8; ++i) dst[i] = zero;
    return;
  }
  if (c == 0) samples_full<0>(g, frame, by, bx, d);
  else if (s420) c == 1 ? samples_420<1>(g, frame, by, bx, d) : samples_420<2>(g, frame, by, bx, d);
  else c == 1 ? samples_full<1>(g, frame, by, bx, d) : samples_full<2>(g, frame, by, bx, d);
#pragma unroll
  for (int i = 0; i < 64; ++i) d[i] -= 128;
#pragma unroll
  for (int y = 0; y < 8; ++y) fdct8<true, 1>(d + 8 * y);
#pragma unroll
  for (int x = 0; x < 8; ++x) fdct8<false, 8>(d + x);
  const unsigned short* div = divisor + (c ? 64 : 0);
#pragma unroll
  for (int i = 0; i < 64; ++i) d[i] = quantise(d[i], div[i]);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    Int4 v;
    v.x = (d[zigzag[8 * i]] & 0xFFFF) | (int)((unsigned int)d[zigzag[8 * i + 1]] << 16);
    v.y = (d[zigzag[8 * i + 2]] & 0xFFFF) | (int)((unsigned int)d[zigzag[8 * i + 3]] << 16);
    v.z = (d[zigzag[8 * i + 4]] & 0xFFFF) | (int)((unsigned int)d[zigzag[8 * i + 5]] << 16);
    v.w = (d[zigzag[8 * i + 6]] & 0xFFFF) | (int)((unsigned int)d[zigzag[8 * i + 7]] << 16);
    dst[i] = v;
  }
}

// ---- entropy: counting and emitting one segment --------------------------------------------------------------------------------
T3D_ENC_LANE unsigned int bswap32(unsigned int v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }
T3D_ENC_LANE int nbits(int v) {          // bits of |v|, |v| < 2^16
  unsigned int a = (unsigned int)(v < 0 ? -v : v);
  int n = 0;
#pragma unroll
  for (int s = 8; s; s >>= 1)
    if (a >> s) a >>= s, n += s;
  return n + (int)a;                     // a is now 0 or 1
}

// The bits of one lane.  EMIT false: only their number.  EMIT true: they go to the frame's unstuffed stream from bit `pos` on,
// MSB first, as 32-bit words (byte-swapped: the stream is a byte sequence); a word the lane fills alone is a plain store, its
// first word when it begins inside it and its last partial word are OR-ed in, since the neighbouring segments own the rest
// of them (the stream is zeroed in front of the launch); a word index is checked against the share before every store.
template <bool EMIT> struct Sink {
  unsigned long long acc, bits;
  int nacc;
  bool shared;
  unsigned int* words;
  long long wi, nwords;

  T3D_ENC_LANE void open(unsigned int* stream, long long nwords_, unsigned long long pos) {
    acc = 0, bits = 0, words = stream, nwords = nwords_, wi = (long long)(pos >> 5), nacc = (int)(pos & 31), shared = nacc != 0;
  }
  T3D_ENC_LANE void put(unsigned int v, int n) {        // n <= 26 bits, v < 2^n
    bits += (unsigned int)n;
    if (!EMIT) return;
    acc = (acc << n) | v;
    nacc += n;
    if (nacc >= 32) {
      nacc -= 32;
      const unsigned int word = bswap32((unsigned int)(acc >> nacc));
      if (wi >= 0 && wi < nwords) {
        if (shared) T3D_ENC_OR(words + wi, word);
        else words[wi] = word;
      }
      shared = false;
      ++wi;
    }
  }
  T3D_ENC_LANE void close() {
    if (!EMIT || nacc == 0) return;
    const unsigned int word = bswap32((unsigned int)(acc << (32 - nacc)));
    if (wi >= 0 && wi < nwords) T3D_ENC_OR(words + wi, word);
    nacc = 0;
  }
};

// a value's code: the symbol's code, then the n low bits of v (v - 1 for a negative v)
template <bool EMIT> T3D_ENC_LANE void put_value(Sink<EMIT>& s, const unsigned int* table, int high, int v) {
  const int n = nbits(v);
  const unsigned int e = table[((high << 4) | n) & 255], extra = (unsigned int)(v < 0 ? v - 1 : v) & ((1u << n) - 1u);
  s.put(((e & 0xFFFFu) << n) | extra, (int)(e >> 16 & 31) + n);
}

// Segment s of a frame (s < g.nseg): the codes of its MCUs [s * seg_mcus, ...).  huff: [4][256] = DC 0, DC 1, AC 0, AC 1.
// EMIT: `pos` is the segment's bit offset, `total` the frame's bit count (the last segment pads the last byte with 1 bits).
// -> the segment's bit count (without the padding)
template <bool EMIT>
T3D_ENC_LANE unsigned long long walk_segment(const Geo& g, const short* coef, const unsigned int* huff, int s, unsigned int* stream,
                                             unsigned long long pos, unsigned long long total) {
  Sink<EMIT> sink;
  sink.open(stream, g.ushare / 4, pos);
  const int ybl = g.bpm - 2;
  const int m0 = s * g.seg_mcus, m1 = g.nmcu - m0 > g.seg_mcus ? m0 + g.seg_mcus : g.nmcu;      // s < nseg: m0 < nmcu
  int pred[3] = {0, 0, 0};
  if (m0 > 0) {                                         // the last block of each component in the MCU in front
    const short* prev = coef + (long long)(m0 - 1) * g.bpm * 64;
    pred[0] = prev[(ybl - 1) * 64], pred[1] = prev[ybl * 64], pred[2] = prev[(ybl + 1) * 64];
  }
  for (long long blk = (long long)m0 * g.bpm, b = 0; blk < (long long)m1 * g.bpm; ++blk, b = b + 1 == g.bpm ? 0 : b + 1) {
    const int c = b < ybl ? 0 : (int)b - ybl + 1, t = c ? 1 : 0;
    const unsigned int* hd = huff + 256 * t;
    const unsigned int* ha = huff + 256 * (2 + t);
    const Int4* src = reinterpret_cast<const Int4*>(coef + blk * 64);
    int run = 0;
    for (int r = 0; r < 8; ++r) {
      const Int4 q = src[r];
      const int pair[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int v = (j & 1) ? pair[j >> 1] >> 16 : (int)(short)(pair[j >> 1] & 0xFFFF);
        if (r == 0 && j == 0) {
          put_value(sink, hd, 0, v - pred[c]);
          pred[c] = v;
        } else if (v == 0) {
          ++run;
        } else {
          for (; run > 15; run -= 16) sink.put(ha[0xF0] & 0xFFFFu, (int)(ha[0xF0] >> 16 & 31));
          put_value(sink, ha, run, v);
          run = 0;
        }
      }
    }
    if (run) sink.put(ha[0] & 0xFFFFu, (int)(ha[0] >> 16 & 31));
  }
  const unsigned long long bits = sink.bits;
  if (EMIT && s == g.nseg - 1) {
    const int pad = (int)((8 - (total & 7)) & 7);
    sink.put((1u << pad) - 1u, pad);
  }
  sink.close();
  return bits;
}

// ---- stuffing ------------------------------------------------------------------------------------------------------------------
// a frame's unstuffed scan in bytes from its bit count, or -1: it does not fit the frame's share of the work buffer
T3D_ENC_LANE long long scan_bytes(const Geo& g, unsigned long long total_bits) {
  const unsigned long long ub = (total_bits + 7) >> 3;
  return ub <= (unsigned long long)g.ushare ? (long long)ub : -1;
}

// a frame's result row; nff: the FF bytes of its unstuffed scan (not looked at when the scan did not fit)
T3D_ENC_LANE t3d_jpeg_enc_result frame_result(const Geo& g, unsigned long long total_bits, unsigned int nff) {
  t3d_jpeg_enc_result res;
  const long long ub = scan_bytes(g, total_bits), least = kHeaderBytes + (long long)((total_bits + 7) >> 3) + 2;
  res.overflow = ub < 0 || least + nff > g.cap;
  res.bytes = res.overflow ? least : least + nff;
  res.reserved = 0;
  return res;
}

T3D_ENC_LANE int count_ff(unsigned int x) {               // bytes of x that are FF
  unsigned int m = ((x & 0x7F7F7F7Fu) + 0x01010101u) & x & 0x80808080u, n = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) n += (m >> (8 * i + 7)) & 1u;
  return (int)n;
}

// FF bytes of chunk c of a frame's unstuffed stream (c < g.nchunk; bytes behind the scan's end are zero)
T3D_ENC_LANE unsigned int chunk_ff(const unsigned int* stream, long long c) {
  const Int4* p = reinterpret_cast<const Int4*>(stream + c * (kChunk / 4));
  int n = 0;
#pragma unroll
  for (int i = 0; i < kChunk / 16; ++i) {
    const Int4 v = p[i];
    n += count_ff((unsigned int)v.x) + count_ff((unsigned int)v.y) + count_ff((unsigned int)v.z) + count_ff((unsigned int)v.w);
  }
  return (unsigned int)n;
}

// chunk c of a frame whose file fits its slot: its bytes (those below `ubytes`, the scan's unstuffed length) to `dst`, the
// place behind the header plus 64 c plus the FF bytes in front of the chunk, a 00 behind every FF
T3D_ENC_LANE void scatter_chunk(const unsigned int* stream, long long c, long long ubytes, unsigned char* dst) {
  const int n = (int)lo((long long)kChunk, ubytes - c * kChunk);
  const Int4* p = reinterpret_cast<const Int4*>(stream + c * (kChunk / 4));
  int o = 0;
#pragma unroll
  for (int i = 0; i < kChunk / 16; ++i) {
    const Int4 v = p[i];
    const unsigned int w4[4] = {(unsigned int)v.x, (unsigned int)v.y, (unsigned int)v.z, (unsigned int)v.w};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      if (16 * i + k < n) {
        const unsigned int b = (w4[k >> 2] >> (8 * (k & 3))) & 255u;
        dst[o++] = (unsigned char)b;
        if (b == 255u) dst[o++] = 0;
      }
    }
  }
}

}  // namespace t3d_jpeg_enc
