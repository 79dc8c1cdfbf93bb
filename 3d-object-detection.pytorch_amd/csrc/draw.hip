// The drawing stage of the live loop (scripts/demo.py:26-46 draw_detections, utils/utils.py:247-270 draw_kp of the reference)
// on the device: rectangles, box edges, keypoint discs, label plates and label text on frames [S][H][W][3] uint8, in place,
// one launch for all cameras (include/t3d.h: t3d_draw_overlays_u8, t3d_draw_glyphs).
//
// OpenCV and objectron.graphics are not available, so the raster rules are this project's own: every
// coverage test is integer arithmetic, restated in numpy by tests/draw_ref.py, and the kernel is bit-equal to that.  The
// look -- colours, thickness, the font below -- is unpinned against the reference's output.
//
// Shape: a 256-thread workgroup owns a 64 x 16 pixel tile, a thread four consecutive pixels of one row.  Camera s has
// 24 * count[s] primitive SLOTS (object t, layer k -> slot 24 t + k; a higher slot is painted later).
//   phase 1  the threads stride over the slots, test each primitive's bounding box against the tile and set one bit per
//            hit in an LDS bitmask (<= 24 * 1024 bits = 3 KB).  Bits, not an appended list: the mask does not depend on
//            the order in which the threads arrive.
//   exit     no bit set: the workgroup returns without touching the frame -- the cost follows the tiles the overlays
//            touch, not S * H * W.
//   phase 2  every thread walks the set bits from the highest down and stops for a pixel at the first primitive that
//            covers it: painter's order without overdraw.  The walk is the same in every lane, so the slot is made a
//            scalar and the primitive is decoded once per wave.
// A thread writes only bytes of its own pixels, so there are no global atomics and nothing depends on scheduling.
#include <string.h>

#include "box_geometry.h"

namespace {

constexpr int kDrawThreads = 256;
constexpr int kTileW = 64, kTileH = 16;       // 16 threads x 4 pixels across, 16 rows
constexpr int kSlots = 24;                    // per object: rectangle, 12 edges, 9 discs, plate, text
constexpr int kMaxT = 1024;
constexpr int kMaskWords = kSlots * kMaxT / 32;
constexpr int kMaxCoord = 8191;
constexpr int kNumGlyphs = 38;                // a-z, 0-9, '_', ' '
constexpr int kFilledGlyph = kNumGlyphs;      // any other character

// The font: 5 x 7, one byte per row, column c at bit 4 - c (the literals read as the glyph looks).  ONE table: the host copy
// serves t3d_draw_glyphs (and through it the numpy restatement), the device copy the kernel.
#define T3D_G(a, b, c, d, e, f, g) {0b##a, 0b##b, 0b##c, 0b##d, 0b##e, 0b##f, 0b##g}
#define T3D_GLYPHS                                                        \
  T3D_G(00000, 00000, 01110, 00001, 01111, 10001, 01111), /* a */         \
  T3D_G(10000, 10000, 10110, 11001, 10001, 10001, 11110), /* b */         \
  T3D_G(00000, 00000, 01110, 10000, 10000, 10001, 01110), /* c */         \
  T3D_G(00001, 00001, 01101, 10011, 10001, 10001, 01111), /* d */         \
  T3D_G(00000, 00000, 01110, 10001, 11111, 10000, 01110), /* e */         \
  T3D_G(00110, 01001, 01000, 11100, 01000, 01000, 01000), /* f */         \
  T3D_G(00000, 01111, 10001, 10001, 01111, 00001, 01110), /* g */         \
  T3D_G(10000, 10000, 10110, 11001, 10001, 10001, 10001), /* h */         \
  T3D_G(00100, 00000, 01100, 00100, 00100, 00100, 01110), /* i */         \
  T3D_G(00010, 00000, 00110, 00010, 00010, 10010, 01100), /* j */         \
  T3D_G(10000, 10000, 10010, 10100, 11000, 10100, 10010), /* k */         \
  T3D_G(01100, 00100, 00100, 00100, 00100, 00100, 01110), /* l */         \
  T3D_G(00000, 00000, 11010, 10101, 10101, 10001, 10001), /* m */         \
  T3D_G(00000, 00000, 10110, 11001, 10001, 10001, 10001), /* n */         \
  T3D_G(00000, 00000, 01110, 10001, 10001, 10001, 01110), /* o */         \
  T3D_G(00000, 11110, 10001, 10001, 11110, 10000, 10000), /* p */         \
  T3D_G(00000, 01111, 10001, 10001, 01111, 00001, 00001), /* q */         \
  T3D_G(00000, 00000, 10110, 11001, 10000, 10000, 10000), /* r */         \
  T3D_G(00000, 00000, 01110, 10000, 01110, 00001, 11110), /* s */         \
  T3D_G(01000, 01000, 11100, 01000, 01000, 01001, 00110), /* t */         \
  T3D_G(00000, 00000, 10001, 10001, 10001, 10011, 01101), /* u */         \
  T3D_G(00000, 00000, 10001, 10001, 10001, 01010, 00100), /* v */         \
  T3D_G(00000, 00000, 10001, 10001, 10101, 10101, 01010), /* w */         \
  T3D_G(00000, 00000, 10001, 01010, 00100, 01010, 10001), /* x */         \
  T3D_G(00000, 10001, 10001, 10001, 01111, 00001, 01110), /* y */         \
  T3D_G(00000, 00000, 11111, 00010, 00100, 01000, 11111), /* z */         \
  T3D_G(01110, 10001, 10011, 10101, 11001, 10001, 01110), /* 0 */         \
  T3D_G(00100, 01100, 00100, 00100, 00100, 00100, 01110), /* 1 */         \
  T3D_G(01110, 10001, 00001, 00010, 00100, 01000, 11111), /* 2 */         \
  T3D_G(11111, 00010, 00100, 00010, 00001, 10001, 01110), /* 3 */         \
  T3D_G(00010, 00110, 01010, 10010, 11111, 00010, 00010), /* 4 */         \
  T3D_G(11111, 10000, 11110, 00001, 00001, 10001, 01110), /* 5 */         \
  T3D_G(00110, 01000, 10000, 11110, 10001, 10001, 01110), /* 6 */         \
  T3D_G(11111, 00001, 00010, 00100, 01000, 01000, 01000), /* 7 */         \
  T3D_G(01110, 10001, 10001, 01110, 10001, 10001, 01110), /* 8 */         \
  T3D_G(01110, 10001, 10001, 01111, 00001, 00010, 01100), /* 9 */         \
  T3D_G(00000, 00000, 00000, 00000, 00000, 00000, 11111), /* _ */         \
  T3D_G(00000, 00000, 00000, 00000, 00000, 00000, 00000)  /* space */

const unsigned char h_glyphs[kNumGlyphs][7] = {T3D_GLYPHS};
__constant__ unsigned char c_glyphs[kNumGlyphs][7] = {T3D_GLYPHS};
#undef T3D_GLYPHS
#undef T3D_G

// OBJECTRON_CLASSES (utils/utils.py of the reference), zero-terminated
__constant__ char c_class_names[9][12] = {"bike", "book", "bottle", "cereal_box", "camera", "chair", "cup", "laptop", "shoe"};

enum { P_NONE = 0, P_RECT, P_SEG, P_DISC, P_FILL, P_TEXT };
enum { C_RECT = 0, C_RECT_OFF, C_EDGE_X, C_EDGE_Y, C_EDGE_Z, C_KP, C_PLATE, C_TEXT, C_COUNT };

struct DrawArgs {
  unsigned char* frames;
  int S, H, W, T;
  const int* count;
  const int* boxes;
  const double* kp;
  const int* ids;
  const int* labels;
  const int* label_count;
  int label_stride;
  int dwords;                // frames 4-byte aligned and W % 4 == 0: a thread's four pixels are three aligned dwords
  t3d_draw_style st;
};

// One primitive.  P_RECT: the box (x0, y0, x1, y1), th; P_SEG: a = (x0, y0), b = (x1, y1), th; P_DISC: centre (x0, y0),
// radius th; P_FILL: the closed rectangle; P_TEXT: origin (x0, y0), th = font scale, n characters of which the first nc are
// the class name of `label`, then a space and the decimal digits of `id`.
struct Prim { int kind, x0, y0, x1, y1, th, col, n, nc, label, id; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// P_i = (rint(x), rint(y)), round half even; valid when both are finite and |.| <= 8191 (NaN and inf fail the comparison)
__device__ __forceinline__ bool draw_point(const double* kp, int i, int& x, int& y) {
  const double fx = rint(kp[2 * i]), fy = rint(kp[2 * i + 1]);
  if (!(fabs(fx) <= (double)kMaxCoord) || !(fabs(fy) <= (double)kMaxCoord)) return false;
  x = (int)fx;
  y = (int)fy;
  return true;
}

__device__ Prim decode_slot(const DrawArgs& a, int s, int slot) {
  Prim p;
  p.kind = P_NONE;
  p.x0 = p.y0 = p.x1 = p.y1 = p.th = p.col = p.n = p.nc = 0;
  p.label = p.id = -1;
  const int t = slot / kSlots, k = slot - t * kSlots;
  const size_t o = (size_t)s * a.T + t;
  const int id = a.ids ? a.ids[o] : -1;
  const bool off = a.ids && id < 0;
  if (k >= 1 && k <= 21) {                                          // edges and discs
    if (off) return p;
    const double* kp = a.kp + o * 18;
    if (k <= 12) {
      const int e = k - 1;
      if (!draw_point(kp, c_edges[e][0], p.x0, p.y0) || !draw_point(kp, c_edges[e][1], p.x1, p.y1)) return p;
      p.kind = P_SEG; p.th = a.st.edge_th; p.col = C_EDGE_X + (e >> 2);
    } else {
      if (!draw_point(kp, k - 13, p.x0, p.y0)) return p;
      p.kind = P_DISC; p.th = a.st.kp_radius; p.col = C_KP;
    }
    return p;
  }
  int bx0 = 0, by0 = 0, bx1 = 0, by1 = 0;
  if (a.boxes) {                                                    // clamped, then ordered
    const int* b = a.boxes + o * 4;
    const int l = clampi(b[0], -kMaxCoord - 1, kMaxCoord), tp = clampi(b[1], -kMaxCoord - 1, kMaxCoord);
    const int r = clampi(b[2], -kMaxCoord - 1, kMaxCoord), bt = clampi(b[3], -kMaxCoord - 1, kMaxCoord);
    bx0 = l < r ? l : r; bx1 = l < r ? r : l;
    by0 = tp < bt ? tp : bt; by1 = tp < bt ? bt : tp;
  }
  if (k == 0) {
    if (!a.boxes) return p;
    p.kind = P_RECT; p.x0 = bx0; p.y0 = by0; p.x1 = bx1; p.y1 = by1; p.th = a.st.rect_th; p.col = off ? C_RECT_OFF : C_RECT;
    return p;
  }
  // plate (k == 22) and text (k == 23)
  int label = -1;
  if (a.labels) {
    const int lc = a.label_count ? clampi(a.label_count[s], 0, a.label_stride) : a.label_stride;
    if (t < lc) label = a.labels[(size_t)s * a.label_stride + t];
  }
  int nc = 0, n;
  if (label >= 0 && label < 9)
    while (c_class_names[label][nc]) ++nc;
  n = nc;
  if ((a.st.flags & T3D_DRAW_IDS) && id >= 0) {
    n += 2;                                                         // the space and the first digit
    for (unsigned v = (unsigned)id; v >= 10; v /= 10) ++n;
  }
  if (n == 0) return p;
  const int ks = a.st.font_scale;
  const int px = a.boxes ? bx0 : 0;
  int py = 0;
  if (a.boxes) py = by0 - 9 * ks > 0 ? by0 - 9 * ks : 0;
  if (k == 22) {
    p.kind = P_FILL; p.x0 = px; p.y0 = py; p.x1 = px + (6 * n - 1) * ks + 2 * ks - 1; p.y1 = py + 9 * ks - 1; p.col = C_PLATE;
  } else {
    p.kind = P_TEXT; p.x0 = px + ks; p.y0 = py + ks; p.th = ks; p.col = C_TEXT; p.n = n; p.nc = nc; p.label = label; p.id = id;
  }
  return p;
}

// closed bounding box of everything the primitive can cover
__device__ __forceinline__ void prim_bbox(const Prim& p, int& lx, int& ly, int& hx, int& hy) {
  switch (p.kind) {
    case P_RECT:
      lx = p.x0 - p.th / 2; ly = p.y0 - p.th / 2; hx = p.x1 + (p.th - 1) / 2; hy = p.y1 + (p.th - 1) / 2;
      break;
    case P_SEG: {
      const int m = (p.th + 1) / 2;                                 // 4 d^2 <= th^2  ->  d <= th / 2
      lx = (p.x0 < p.x1 ? p.x0 : p.x1) - m; hx = (p.x0 < p.x1 ? p.x1 : p.x0) + m;
      ly = (p.y0 < p.y1 ? p.y0 : p.y1) - m; hy = (p.y0 < p.y1 ? p.y1 : p.y0) + m;
      break;
    }
    case P_DISC:
      lx = p.x0 - p.th; hx = p.x0 + p.th; ly = p.y0 - p.th; hy = p.y0 + p.th;
      break;
    case P_FILL:
      lx = p.x0; ly = p.y0; hx = p.x1; hy = p.y1;
      break;
    default:                                                        // P_TEXT
      lx = p.x0; ly = p.y0; hx = p.x0 + 6 * p.n * p.th - 1; hy = p.y0 + 7 * p.th - 1;
      break;
  }
}

__device__ __forceinline__ int glyph_of(char c) {
  if (c >= 'a' && c <= 'z') return c - 'a';
  if (c >= '0' && c <= '9') return 26 + (c - '0');
  if (c == '_') return 36;
  if (c == ' ') return 37;
  return kFilledGlyph;
}

__device__ __forceinline__ bool prim_covers(const Prim& p, int x, int y) {
  switch (p.kind) {
    case P_RECT: {
      const int h0 = p.th / 2, h1 = (p.th - 1) / 2;
      const bool outer = x >= p.x0 - h0 && x <= p.x1 + h1 && y >= p.y0 - h0 && y <= p.y1 + h1;
      const bool inner = x >= p.x0 + h1 + 1 && x <= p.x1 - h0 - 1 && y >= p.y0 + h1 + 1 && y <= p.y1 - h0 - 1;
      return outer && !inner;
    }
    case P_SEG: {
      const long long abx = p.x1 - p.x0, aby = p.y1 - p.y0, apx = x - p.x0, apy = y - p.y0;
      const long long L2 = abx * abx + aby * aby, dot = apx * abx + apy * aby, th2 = (long long)p.th * p.th;
      if (L2 == 0 || dot <= 0) return 4 * (apx * apx + apy * apy) <= th2;
      if (dot >= L2) {
        const long long bpx = x - p.x1, bpy = y - p.y1;
        return 4 * (bpx * bpx + bpy * bpy) <= th2;
      }
      const long long cross = apx * aby - apy * abx;
      return 4 * cross * cross <= th2 * L2;
    }
    case P_DISC: {
      const long long dx = x - p.x0, dy = y - p.y0;
      return dx * dx + dy * dy <= (long long)p.th * p.th;
    }
    case P_FILL:
      return x >= p.x0 && x <= p.x1 && y >= p.y0 && y <= p.y1;
    case P_TEXT: {
      if (x < p.x0 || y < p.y0) return false;
      const int cx = (x - p.x0) / p.th, cy = (y - p.y0) / p.th;
      if (cx >= 6 * p.n || cy >= 7) return false;
      const int ci = cx / 6, col = cx - ci * 6;
      if (col >= 5) return false;
      char c;
      if (ci < p.nc) {
        c = c_class_names[p.label][ci];
      } else if (ci == p.nc) {
        c = ' ';
      } else {
        unsigned v = (unsigned)p.id;
        for (int d = p.n - 1 - ci; d > 0; --d) v /= 10;
        c = (char)('0' + v % 10);
      }
      const int g = glyph_of(c);
      const unsigned row = g == kFilledGlyph ? 0x1fu : c_glyphs[g][cy];
      return (row >> (4 - col)) & 1u;
    }
    default:
      return false;
  }
}

// phase 1 of thread `tid`: its share of the camera's slots against the tile [X0, X1] x [Y0, Y1]; true when it set a bit
__device__ __forceinline__ bool mark_slots(const DrawArgs& a, int s, int tid, int nslots, int X0, int Y0, int X1, int Y1,
                                           unsigned* mask) {
  bool hit = false;
  for (int slot = tid; slot < nslots; slot += kDrawThreads) {
    const Prim p = decode_slot(a, s, slot);
    if (p.kind == P_NONE) continue;
    int lx, ly, hx, hy;
    prim_bbox(p, lx, ly, hx, hy);
    if (lx <= X1 && hx >= X0 && ly <= Y1 && hy >= Y0) {
      atomicOr(&mask[slot >> 5], 1u << (slot & 31));
      hit = true;
    }
  }
  return hit;
}

// phase 2 of thread `tid`: the topmost covering primitive of each of its four pixels, then the stores
__device__ __forceinline__ void paint_pixels(const DrawArgs& a, int s, int tid, int X0, int Y0, int nwords, const unsigned* mask,
                                             const unsigned* colour) {
  const int x = X0 + (tid & 15) * 4, y = Y0 + (tid >> 4);
  if (x >= a.W || y >= a.H) return;
  const int npix = a.W - x < 4 ? a.W - x : 4;
  const unsigned want = (1u << npix) - 1u;
  unsigned covered = 0u, rgb0 = 0u, rgb1 = 0u, rgb2 = 0u, rgb3 = 0u;
  for (int w = nwords - 1; w >= 0 && covered != want; --w) {
    unsigned m = __builtin_amdgcn_readfirstlane(mask[w]);           // every lane reads the same word
    while (m && covered != want) {
      const int b = 31 - __clz((int)m);
      m &= ~(1u << b);
      // (the lanes still in the loop have removed the same bits from the same word: the slot is wave-uniform)
      const Prim p = decode_slot(a, s, __builtin_amdgcn_readfirstlane(w * 32 + b));
      const unsigned c = colour[p.col];
      if (!(covered & 1u) && prim_covers(p, x, y)) { covered |= 1u; rgb0 = c; }
      if (npix > 1 && !(covered & 2u) && prim_covers(p, x + 1, y)) { covered |= 2u; rgb1 = c; }
      if (npix > 2 && !(covered & 4u) && prim_covers(p, x + 2, y)) { covered |= 4u; rgb2 = c; }
      if (npix > 3 && !(covered & 8u) && prim_covers(p, x + 3, y)) { covered |= 8u; rgb3 = c; }
    }
  }
  if (!covered) return;
  unsigned char* q = a.frames + (((size_t)s * a.H + y) * a.W + x) * 3;
  if (a.dwords) {
    // W % 4 == 0: all four pixels exist and their 12 bytes are three aligned dwords owned by this thread alone
    unsigned* d = reinterpret_cast<unsigned*>(q);
    unsigned d0 = d[0], d1 = d[1], d2 = d[2];
    if (covered & 1u) d0 = (d0 & 0xff000000u) | rgb0;
    if (covered & 2u) { d0 = (d0 & 0x00ffffffu) | (rgb1 << 24); d1 = (d1 & 0xffff0000u) | (rgb1 >> 8); }
    if (covered & 4u) { d1 = (d1 & 0x0000ffffu) | (rgb2 << 16); d2 = (d2 & 0xffffff00u) | (rgb2 >> 16); }
    if (covered & 8u) d2 = (d2 & 0x000000ffu) | (rgb3 << 8);
    d[0] = d0; d[1] = d1; d[2] = d2;
  } else {
    if (covered & 1u) { q[0] = (unsigned char)rgb0; q[1] = (unsigned char)(rgb0 >> 8); q[2] = (unsigned char)(rgb0 >> 16); }
    if (covered & 2u) { q[3] = (unsigned char)rgb1; q[4] = (unsigned char)(rgb1 >> 8); q[5] = (unsigned char)(rgb1 >> 16); }
    if (covered & 4u) { q[6] = (unsigned char)rgb2; q[7] = (unsigned char)(rgb2 >> 8); q[8] = (unsigned char)(rgb2 >> 16); }
    if (covered & 8u) { q[9] = (unsigned char)rgb3; q[10] = (unsigned char)(rgb3 >> 8); q[11] = (unsigned char)(rgb3 >> 16); }
  }
}

__device__ __forceinline__ unsigned pack_colour(const unsigned char* c) {
  return (unsigned)c[0] | ((unsigned)c[1] << 8) | ((unsigned)c[2] << 16);
}

__global__ __launch_bounds__(kDrawThreads) void draw_overlays_kernel(const DrawArgs a) {
  __shared__ unsigned mask[kMaskWords];
  __shared__ unsigned colour[C_COUNT];
  __shared__ int any;
  const int s = blockIdx.z, tid = threadIdx.x;
  const int n = clampi(a.count ? a.count[s] : a.T, 0, a.T);
  if (n == 0) return;                                               // (the same in every thread of the workgroup)
  const int nslots = n * kSlots, nwords = (nslots + 31) >> 5;       // <= kMaskWords: n <= T <= kMaxT
  for (int i = tid; i < nwords; i += kDrawThreads) mask[i] = 0u;
  if (tid == 0) {
    any = 0;
#pragma unroll
    for (int c = 0; c < C_COUNT; ++c) colour[c] = pack_colour(a.st.colors[c]);
  }
  __syncthreads();
  // ---- phase 1: which primitives can touch this tile
  const int X0 = blockIdx.x * kTileW, Y0 = blockIdx.y * kTileH;
  const int X1 = (X0 + kTileW < a.W ? X0 + kTileW : a.W) - 1, Y1 = (Y0 + kTileH < a.H ? Y0 + kTileH : a.H) - 1;
  if (mark_slots(a, s, tid, nslots, X0, Y0, X1, Y1, mask)) any = 1;
  __syncthreads();
  if (!any) return;                                                 // nothing of this camera's overlays meets the tile
  // ---- phase 2 (no barrier below)
  paint_pixels(a, s, tid, X0, Y0, nwords, mask, colour);
}

}  // namespace

// include/t3d.h
extern "C" int t3d_draw_overlays_u8(unsigned char* frames, int S, int H, int W, const int* count, const int* boxes,
                                    const double* kp, const int* ids, const int* labels, const int* label_count, int label_stride,
                                    int T, const t3d_draw_style* style, void* stream) {
  if (!frames || !kp || !style) return T3D_ERR_ARG;
  if (S < 0 || S > 65535 || H < 1 || H > kMaxCoord + 1 || W < 1 || W > kMaxCoord + 1 || T < 1 || T > kMaxT) return T3D_ERR_ARG;
  if (style->rect_th < 1 || style->rect_th > 16 || style->edge_th < 1 || style->edge_th > 16) return T3D_ERR_ARG;
  if (style->kp_radius < 0 || style->kp_radius > 32 || style->font_scale < 1 || style->font_scale > 8) return T3D_ERR_ARG;
  if (labels && (label_stride < 1 || (!label_count && label_stride < T))) return T3D_ERR_ARG;
  if (S == 0) return T3D_OK;
  DrawArgs a{};
  a.frames = frames; a.S = S; a.H = H; a.W = W; a.T = T;
  a.count = count; a.boxes = boxes; a.kp = kp; a.ids = ids; a.labels = labels; a.label_count = label_count;
  a.label_stride = label_stride;
  a.dwords = (reinterpret_cast<uintptr_t>(frames) % 4 == 0 && W % 4 == 0) ? 1 : 0;
  a.st = *style;
  T3D_LAUNCH(draw_overlays_kernel, dim3(cdiv(W, kTileW), cdiv(H, kTileH), S), dim3(kDrawThreads), 0,
             reinterpret_cast<hipStream_t>(stream), a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_draw_glyphs(unsigned char* out, int bytes) {
  const int total = (int)sizeof(h_glyphs);
  if (bytes < 0 || (!out && bytes > 0)) return T3D_ERR_ARG;
  if (bytes > 0) memcpy(out, h_glyphs, bytes < total ? bytes : total);
  return total;
}
