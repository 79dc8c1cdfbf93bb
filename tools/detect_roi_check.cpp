// Host check of the crop-decode planner (csrc/detect_roi.h, what a lane of t3d_detect_roi_plan runs), meant to be built with
// the sanitizers:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/detect_roi_check.cpp -o detect_roi_check
//   ./detect_roi_check [ROUNDS]
//
// Seeded: frames of random size, sampling and seg_mcus with the index row the indexer would write for them, records with every
// turn, pastes and crops inside, across and outside the pasted frame.  Each round plans a batch through t3d_roi::plan_item with
// the records, the sample table, the rows, the items and every output in heap blocks of exactly their sizes, so a read or write
// past one is a sanitizer report.  What comes out of a good record must be a rectangle inside its frame that
// t3d_jpeg_lane::roi_geom -- the check every decode kernel makes -- accepts with the whole-frame totals, and the rewritten record
// must fit its slot.  Then the same with MUTATED inputs: any field of a record, of a row or of an item replaced by a random
// value, the sample table pointing anywhere; nothing is asserted of those results but that planning them is defined behaviour.
// Exit status 0: no invariant failed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../3d-object-detection.pytorch_amd/csrc/detect_roi.h"

namespace L = t3d_jpeg_lane;
namespace P = t3d_roi;

static unsigned long long g_state = 0x9E3779B97F4A7C15ull;
static unsigned long long rnd() {
  g_state ^= g_state << 13, g_state ^= g_state >> 7, g_state ^= g_state << 17;
  return g_state;
}
static int below(int n) { return (int)(rnd() % (unsigned long long)n); }
static int between(int lo, int hi) { return lo + below(hi - lo + 1); }

template <class T> static T* block(int n) { return static_cast<T*>(malloc(n ? sizeof(T) * (size_t)n : 1)); }

static t3d_jpeg_info make_info() {
  t3d_jpeg_info f;
  memset(&f, 0, sizeof f);
  const int big = below(4) == 0;
  f.h = big ? between(1, 65535) : between(1, 300), f.w = big ? between(1, 65535) : between(1, 300);
  f.sampling = below(3), f.ncomp = f.sampling == T3D_JPEG_GRAY ? 1 : 3;
  const int px = f.sampling == T3D_JPEG_420 ? 16 : 8;
  f.mcus_x = (f.w + px - 1) / px, f.mcus_y = (f.h + px - 1) / px;
  f.seg_mcus = between(1, 5);
  f.nseg = (int)(((long long)f.mcus_x * f.mcus_y + f.seg_mcus - 1) / f.seg_mcus);
  f.scan_offset = between(20, 700), f.scan_bytes = between(1, 1 << 20);
  return f;
}

static t3d_det_sample make_record(const t3d_jpeg_info& f, long long offset) {
  t3d_det_sample s;
  memset(&s, 0, sizeof s);
  s.offset = offset, s.h = f.h, s.w = f.w;
  s.turns = below(3) == 0 ? 0 : (below(2) ? 1 : 3);
  const int rw = s.turns ? f.h : f.w, rh = s.turns ? f.w : f.h;
  s.left = below(3) ? between(0, 2 * rw) : 0, s.top = below(3) ? between(0, 2 * rh) : 0;
  const int W = 3 * rw + 2, H = 3 * rh + 2;
  switch (below(4)) {
    case 0: s.cx0 = 0, s.cy0 = 0, s.cx1 = W, s.cy1 = H; break;                                      // the canvas
    case 1: s.cx0 = s.left + below(rw), s.cy0 = s.top + below(rh), s.cx1 = s.cx0 + 1, s.cy1 = s.cy0 + 1; break;      // one pixel
    default:
      s.cx0 = below(W), s.cy0 = below(H);
      s.cx1 = s.cx0 + between(1, W - s.cx0), s.cy1 = s.cy0 + between(1, H - s.cy0);
  }
  s.flags = below(128), s.perm[0] = 2, s.perm[1] = 0, s.perm[2] = 1;
  return s;
}

static int fail(const char* what, int round, int j) {
  fprintf(stderr, "detect_roi_check: round %d item %d: %s\n", round, j, what);
  return 1;
}

int main(int argc, char** argv) {
  const int rounds = argc > 1 ? atoi(argv[1]) : 2000;
  long long planned = 0, parts = 0, empty = 0, passed = 0;
  for (int round = 0; round < 2 * rounds; ++round) {
    const bool mutate = round >= rounds;
    const int B = between(1, 40), n = between(0, B);
    t3d_det_sample* rec = block<t3d_det_sample>(B);
    t3d_det_sample* drawn = block<t3d_det_sample>(B);
    int* sample = block<int>(n);
    t3d_jpeg_info* infos = block<t3d_jpeg_info>(n);
    t3d_jpeg_item* items = block<t3d_jpeg_item>(n);
    t3d_jpeg_item* out = block<t3d_jpeg_item>(n);
    int* rects = block<int>(12 * n);
    int* diag = block<int>(2 * n);
    // records of frames nobody plans (host-decoded ones) first, then one per item, shuffled through the sample table
    long long off = 0, blocks = 0, segs = 0, bytes = 0;
    for (int i = 0; i < B; ++i) {
      const t3d_jpeg_info f = make_info();
      rec[i] = make_record(f, off);
      if (i < n) {
        infos[i] = f, sample[i] = i;
        items[i] = {bytes, f.scan_offset + f.scan_bytes + 2, off, blocks, segs, 0};
        bytes += items[i].file_bytes, segs += f.nseg, blocks += (long long)f.mcus_x * f.mcus_y * t3d_jpeg_mcu_blocks(f.sampling);
      }
      off += (long long)f.h * f.w * 3;
    }
    const long long src_bytes = off;
    for (int j = n - 1; j > 0; --j) {                 // items in another order than their records
      const int k = below(j + 1);
      const t3d_det_sample t = rec[sample[j]];
      rec[sample[j]] = rec[sample[k]], rec[sample[k]] = t;
      const int u = sample[j];
      sample[j] = sample[k], sample[k] = u;
    }
    if (mutate) {
      for (int m = between(1, 6); m > 0; --m) {
        const long long v = below(3) == 0 ? (long long)rnd() : (below(2) ? between(-3, 3) : (long long)(int)rnd());
        switch (n ? below(4) : 0) {
          case 0: reinterpret_cast<int*>(rec + below(B))[below(20)] = (int)v; break;
          case 1: reinterpret_cast<int*>(infos + below(n))[below(14)] = (int)v; break;
          case 2: reinterpret_cast<long long*>(items + below(n))[below(6)] = v; break;
          default: sample[below(n)] = (int)v;
        }
      }
    }
    memcpy(drawn, rec, sizeof(t3d_det_sample) * (size_t)B);
    if (P::check(rec, B, infos, items, n, src_bytes, out, rects, diag) != T3D_OK) return fail("check refused the call", round, -1);
    for (int j = 0; j < n; ++j) P::plan_item(j, rec, B, sample, infos, items, src_bytes, out, rects, diag);
    for (int j = 0; j < n && !mutate; ++j) {
      const t3d_jpeg_info& f = infos[j];
      const t3d_det_sample &s = rec[sample[j]], &d = drawn[sample[j]];
      const int* r = rects + 12 * j;
      if (r[0] < 0 || r[1] < 0 || r[0] >= r[2] || r[1] >= r[3] || r[2] > f.w || r[3] > f.h) return fail("a rectangle outside its frame", round, j);
      if (s.offset != d.offset || s.h != r[3] - r[1] || s.w != r[2] - r[0]) return fail("the record is not the rectangle's", round, j);
      if (!P::det_ok(s, src_bytes)) return fail("the rewritten record would be refused", round, j);
      const long long px = (long long)(r[3] - r[1]) * (r[2] - r[0]);
      if (diag[2 * j] != (px > 0x7fffffffll ? 0x7fffffff : (int)px)) return fail("diag: pixels", round, j);
      // the decode's own check, with the whole-frame totals (it reads nothing: the pointers only take offsets)
      static unsigned char base[1];
      const L::Roi roi = L::roi_geom(base, bytes, &f, reinterpret_cast<const t3d_jpeg_seg*>(base), segs, out[j], r, base, src_bytes, base,
                                     blocks);
      if (!roi.g.ok) return fail("roi_geom refuses the planned item", round, j);
      if (roi.g.nblocks != diag[2 * j + 1]) return fail("diag: blocks", round, j);
      ++planned;
      parts += px < (long long)f.h * f.w, empty += px == 1, passed += px == (long long)f.h * f.w;
    }
    for (int i = n; i < B && !mutate; ++i)            // (before the shuffle the records behind n had no item; the shuffle moved none of them)
      if (memcmp(rec + i, drawn + i, sizeof(t3d_det_sample))) return fail("a record without an item was written", round, i);
    free(rec), free(drawn), free(sample), free(infos), free(items), free(out), free(rects), free(diag);
  }
  printf("detect_roi_check: %lld items planned and accepted by roi_geom (%lld parts, %lld single pixels, %lld whole frames), %d mutated rounds\n",
         planned, parts, empty, passed, rounds);
  return planned > 0 && parts > 0 && empty > 0 && passed > 0 ? 0 : 1;
}
