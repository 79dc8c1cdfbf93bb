// From a drawn detection record to the tables of t3d_jpeg_decode_roi_u8, for ONE sample: the part of the source frame that the
// record's crop reads, its MCU rectangle and segment run, the item read the rectangle entry's way, and the record rewritten
// for the sub-frame (include/t3d.h next to t3d_detect_roi_plan states the contract).  The MCU rule is csrc/jpeg_decode.h's
// roi_mcus, by include.  Like that header it has no HIP include and marks its functions with T3D_JPEG_LANE: csrc/detect_roi.hip
// runs `plan` in a kernel, one sample a lane; csrc/detect_roi_host.hip and tools/detect_roi_check.cpp run it on the CPU.
// Integers only.
#pragma once
#include "jpeg_decode.h"

namespace t3d_roi {

namespace L = t3d_jpeg_lane;

// csrc/detect_augment.hip: det_check.  A record it refuses is a zero image there whatever the frame holds, so the planner
// leaves such a sample as it is.
constexpr int DET_FLAGS = T3D_DET_FLIP | T3D_DET_BRIGHTNESS | T3D_DET_CONTRAST | T3D_DET_CONTRAST_LAST | T3D_DET_HSV |
                          T3D_DET_SATURATION | T3D_DET_HUE;
constexpr int DET_MAX_CROP = 1 << 24;
T3D_JPEG_LANE bool det_ok(const t3d_det_sample& s, long long src_bytes) {
  if (s.h <= 0 || s.w <= 0 || s.offset < 0 || s.offset > src_bytes) return false;
  if ((long long)s.h * s.w > (src_bytes - s.offset) / 3) return false;
  if (s.turns != 0 && s.turns != 1 && s.turns != 3) return false;
  if (s.flags & ~DET_FLAGS) return false;
  const long long cw = (long long)s.cx1 - s.cx0, ch = (long long)s.cy1 - s.cy0;
  if (cw <= 0 || ch <= 0 || cw > DET_MAX_CROP || ch > DET_MAX_CROP) return false;
  const int p0 = s.perm[0], p1 = s.perm[1], p2 = s.perm[2];
  if (p0 < 0 || p0 > 2 || p1 < 0 || p1 > 2 || p2 < 0 || p2 > 2 || p0 == p1 || p0 == p2 || p1 == p2) return false;
  return true;
}

// What the arithmetic below needs of an info row; anything else about it is the decoder's to check (status 2).
T3D_JPEG_LANE bool info_ok(const t3d_jpeg_info& f) {
  if (f.h < 1 || f.w < 1 || f.h > 65535 || f.w > 65535 || f.seg_mcus < 1) return false;
  if (f.sampling != T3D_JPEG_GRAY && f.sampling != T3D_JPEG_444 && f.sampling != T3D_JPEG_420) return false;
  const int px = f.sampling == T3D_JPEG_420 ? 16 : 8;
  return f.mcus_x == (f.w + px - 1) / px && f.mcus_y == (f.h + px - 1) / px;
}

T3D_JPEG_LANE int sat31(long long v) { return v > 0x7fffffffll ? 0x7fffffff : (int)v; }
T3D_JPEG_LANE long long wrap_add(long long a, long long b) { return (long long)((unsigned long long)a + (unsigned long long)b); }

// rec: the sample's record (nullptr: there is none), rewritten in place when a rectangle is planned.  info, whole: the frame's
// index row and the whole-frame item the host planned.  -> item, rect [12], diag [2].
T3D_JPEG_LANE void plan(t3d_det_sample* rec, long long src_bytes, const t3d_jpeg_info& info, const t3d_jpeg_item& whole,
                        t3d_jpeg_item* item, int* rect, int* diag) {
  const bool good = info_ok(info);
  int x0 = 0, y0 = 0, x1 = info.w, y1 = info.h;
  t3d_det_sample s;
  bool rewrite = false;
  if (good && rec) {
    s = *rec;
    rewrite = det_ok(s, src_bytes) && s.h == info.h && s.w == info.w;
  }
  if (rewrite) {
    const int h = s.h, w = s.w;
    const bool turned = s.turns != 0;
    const long long rw = turned ? h : w, rh = turned ? w : h;
    const long long a0 = L::hi((long long)s.cx0 - s.left, 0ll), a1 = L::lo((long long)s.cx1 - s.left, rw);
    const long long b0 = L::hi((long long)s.cy0 - s.top, 0ll), b1 = L::lo((long long)s.cy1 - s.top, rh);
    if (a0 >= a1 || b0 >= b1) {                       // the crop lies wholly in the fill: one pixel, which it does not see
      x0 = y0 = 0, x1 = y1 = 1;
    } else if (s.turns == 0) {
      x0 = (int)a0, x1 = (int)a1, y0 = (int)b0, y1 = (int)b1;
    } else if (s.turns == 1) {                        // turned (xr, yr) is source (w - 1 - yr, xr)
      x0 = (int)(w - b1), x1 = (int)(w - b0), y0 = (int)a0, y1 = (int)a1;
    } else {                                          // turned (xr, yr) is source (yr, h - 1 - xr)
      x0 = (int)b0, x1 = (int)b1, y0 = (int)(h - a1), y1 = (int)(h - a0);
    }
    // the sub-frame lies where it lay in the canvas (a paste beyond the largest int stays outside every crop there)
    const long long dl = s.turns == 0 ? x0 : (s.turns == 1 ? y0 : h - y1), dt = s.turns == 0 ? y0 : (s.turns == 1 ? w - x1 : x0);
    rec->offset = whole.out_offset;
    rec->h = y1 - y0, rec->w = x1 - x0;
    rec->left = sat31((long long)s.left + dl), rec->top = sat31((long long)s.top + dt);
  }
  L::McuRect m;
  m.mx0 = m.my0 = 0, m.mx1 = info.mcus_x, m.my1 = info.mcus_y;
  int seg_first = 0, seg_count = info.nseg;
  if (good) {
    m = L::roi_mcus(info.sampling, info.h, info.w, x0, y0, x1, y1);
    const long long first = ((long long)m.my0 * info.mcus_x + m.mx0) / info.seg_mcus;
    const long long last = ((long long)(m.my1 - 1) * info.mcus_x + m.mx1 - 1) / info.seg_mcus;
    seg_first = (int)first, seg_count = (int)(last - first + 1);
  }
  rect[0] = x0, rect[1] = y0, rect[2] = x1, rect[3] = y1;
  rect[4] = m.mx0, rect[5] = m.my0, rect[6] = m.mx1, rect[7] = m.my1;
  rect[8] = seg_first, rect[9] = seg_count, rect[10] = rect[11] = 0;
  // the whole resident scan; the crop packed at the start of its frame's slot, its blocks at the start of its frame's share
  item->file_offset = wrap_add(whole.file_offset, info.scan_offset);
  item->file_bytes = info.scan_bytes;
  item->out_offset = whole.out_offset;
  item->block_offset = whole.block_offset;
  item->seg_offset = wrap_add(whole.seg_offset, seg_first);
  item->reserved = 0;
  // (a good row: at most 65535 x 65535 pixels and 8192 x 8192 MCUs of six blocks)
  diag[0] = good ? sat31((long long)(y1 - y0) * (x1 - x0)) : 0;
  diag[1] = good ? sat31((long long)(m.my1 - m.my0) * (m.mx1 - m.mx0) * t3d_jpeg_mcu_blocks(info.sampling)) : 0;
}

// What both entry points check of their arguments -> T3D_OK or T3D_ERR_ARG.
inline int check(const void* records, int B, const void* infos, const void* items, int n, long long src_bytes, const void* roi_items,
                 const void* rects, const void* diag) {
  if (B < 0 || B > 65535 || n < 0 || n > 65535 || src_bytes < 0) return T3D_ERR_ARG;
  if (n && (!records || !infos || !items || !roi_items || !rects || !diag)) return T3D_ERR_ARG;
  return T3D_OK;
}

// item j of the call
T3D_JPEG_LANE void plan_item(int j, void* records, int B, const int* sample, const t3d_jpeg_info* infos, const t3d_jpeg_item* items,
                             long long src_bytes, t3d_jpeg_item* roi_items, int* rects, int* diag) {
  const int i = sample ? sample[j] : j;
  t3d_det_sample* rec = i >= 0 && i < B ? static_cast<t3d_det_sample*>(records) + i : nullptr;
  plan(rec, src_bytes, infos[j], items[j], roi_items + j, rects + 12ll * j, diag + 2ll * j);
}

}  // namespace t3d_roi
