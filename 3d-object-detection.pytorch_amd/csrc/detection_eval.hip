// COCO bbox evaluation of the detector on the device: the per-image half of the published pycocotools COCOeval
// (iouType = 'bbox') as mmdet 2.x's CocoDataset.evaluate(metric='bbox') drives it for
// configs/detection/mnv2_ssd_300_2_heads.py:56-60,130-143.  The record these kernels fill is read back once per epoch and
// accumulated / summarised on the host (torchdet3d/evaluation/detection_eval.py).
//
// PARITY UNPINNED: pycocotools is not installed anywhere this project is built.  DESIGN.md section 7 ("COCO bbox evaluation
// protocol") states the protocol; that statement is the definition, tests/coco_eval_ref.py is its plain-loop numpy form.
// Stated deviations: no crowd branch (the reference's converter writes iscrowd = 0 for every annotation and the loader drops
// crowd boxes), NMS runs at input scale before the rescale to the original frame (mmdet rescales first), and boxes never
// make the xyxy -> xywh -> JSON -> xyxy round trip.
//
//   t3d_ssd_cap_per_image  one 256-thread workgroup per image: the scores of the image's valid rows go to LDS, a thread per
//     row counts the rows that sort before it (score descending, class ascending, NMS order ascending), and a thread per
//     class counts its survivors.  `out` is only read.
//   t3d_coco_match         one 256-thread workgroup per (image, class): all threads scale the boxes to the original frame and
//     fill the D x G IoU matrix in LDS (fp64, D <= 100, G <= 64: 51 200 bytes); then wave 0 runs the greedy matching, lane
//     a * 10 + t owning (area range a, threshold t) with its matched ground truths as one 64-bit mask in registers, and the
//     40 lanes' verdicts on a detection are gathered into the record's words with a ballot.  Plain stores, one owner per
//     cell, no atomics: two runs are bit-identical.
#include "common.h"

namespace {

constexpr int MAX_DET = 100, MAX_GT = 64, NTHR = 10, NAREA = 4, NPAIR = NAREA * NTHR;
constexpr int CAP_MAX_ROWS = 4096;

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// numpy's stable argsort of -score: a larger score first, nan last, equal keys in row order
__device__ __forceinline__ bool sorts_before(float sj, int j, float si, int i) {
  const bool nj = sj != sj, ni = si != si;
  if (nj || ni) return nj == ni ? j < i : ni;
  return sj > si || (sj == si && j < i);
}

__global__ __launch_bounds__(256) void ssd_cap_kernel(const float* __restrict__ out, const int* __restrict__ counts, int nc, int K,
                                                      int max_per_img, int* __restrict__ counts_out) {
  __shared__ float s_score[CAP_MAX_ROWS];
  __shared__ unsigned char s_keep[CAP_MAX_ROWS];
  __shared__ int s_start[CAP_MAX_ROWS + 1];        // rows of class c are s_start[c] .. s_start[c + 1] of the image's valid rows
  const int b = blockIdx.x, tid = threadIdx.x;
  const int* cnt = counts + (size_t)b * nc;
  if (tid == 0) {
    int s = 0;
    for (int c = 0; c < nc; ++c) {
      s_start[c] = s;
      s += clampi(cnt[c], K);
    }
    s_start[nc] = s;
  }
  __syncthreads();
  const int total = s_start[nc];
  for (int c = 0; c < nc; ++c) {
    const int lo = s_start[c], hi = s_start[c + 1];
    for (int i = lo + tid; i < hi; i += 256) s_score[i] = out[(((size_t)b * nc + c) * K + (i - lo)) * 6 + 4];
  }
  __syncthreads();
  for (int i = tid; i < total; i += 256) {
    const float si = s_score[i];
    int rank = 0;
    for (int j = 0; j < total; ++j) rank += sorts_before(s_score[j], j, si, i);
    s_keep[i] = rank < max_per_img;
  }
  __syncthreads();
  // one thread per class: its survivors (a prefix of the class when its rows are in non-increasing score order)
  for (int c = tid; c < nc; c += 256) {
    int keep = 0;
    for (int i = s_start[c]; i < s_start[c + 1]; ++i) keep += s_keep[i];
    counts_out[(size_t)b * nc + c] = keep;
  }
}

struct MatchSmem {
  double iou[MAX_DET * MAX_GT];     // row d, column g of the cell's compacted ground truths; stride = their number
  double dbox[MAX_DET][4], darea[MAX_DET];
  double gbox[MAX_GT][4], garea[MAX_GT];
  int gslot[MAX_GT];
  unsigned char order[NAREA][MAX_GT];      // per area range: the non-ignored ground truths in slot order, then the ignored ones
  int nnon[NAREA];
  int ng;
};

__global__ __launch_bounds__(256) void coco_match_kernel(const float* __restrict__ out, const int* __restrict__ counts, int nc, int K,
                                                         const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                         const int* __restrict__ gt_counts, int G, const int* __restrict__ ori_shapes,
                                                         int in_w, int in_h, const double* __restrict__ iou_thrs,
                                                         const double* __restrict__ area_rngs, int base,
                                                         float* __restrict__ rec_score, unsigned long long* __restrict__ rec_dtm,
                                                         unsigned long long* __restrict__ rec_dtig, int* __restrict__ rec_ndt,
                                                         int* __restrict__ rec_ngt, int* __restrict__ rec_valid) {
  __shared__ MatchSmem sm;
  const int b = blockIdx.x / nc, c = blockIdx.x % nc, tid = threadIdx.x;
  const int h = ori_shapes[2 * b], w = ori_shapes[2 * b + 1];
  const bool ok = h > 0 && w > 0;
  const double fx = (double)w / (double)in_w, fy = (double)h / (double)in_h;
  const size_t cell = ((size_t)base + b) * nc + c;
  const int nd = ok ? min(clampi(counts[(size_t)b * nc + c], K), MAX_DET) : 0;
  const float* rows = out + ((size_t)b * nc + c) * K * 6;

  // ---- the cell's ground truths, compacted in slot order (the validity rule of t3d_ssd_multibox_loss)
  if (tid == 0) {
    int n = 0;
    const int cnt = ok ? clampi(gt_counts[b], G) : 0;
    for (int g = 0; g < cnt; ++g) {
      const float* p = gt_boxes + ((size_t)b * G + g) * 4;
      const float x1 = p[0], y1 = p[1], x2 = p[2], y2 = p[3];
      const int lab = gt_labels[(size_t)b * G + g];
      if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2)) || !(x2 > x1) || !(y2 > y1) || lab != c) continue;
      sm.gslot[n++] = g;
    }
    sm.ng = n;
    if (c == 0) rec_valid[(size_t)base + b] = ok;
    rec_ndt[cell] = nd;
  }
  __syncthreads();
  const int ng = sm.ng;
  for (int g = tid; g < ng; g += 256) {
    const float* p = gt_boxes + ((size_t)b * G + sm.gslot[g]) * 4;
    const double x1 = (double)p[0] * fx, y1 = (double)p[1] * fy, x2 = (double)p[2] * fx, y2 = (double)p[3] * fy;
    sm.gbox[g][0] = x1; sm.gbox[g][1] = y1; sm.gbox[g][2] = x2; sm.gbox[g][3] = y2;
    sm.garea[g] = (x2 - x1) * (y2 - y1);
  }
  for (int d = tid; d < MAX_DET; d += 256) {
    float score = 0.f;
    if (d < nd) {
      const float* p = rows + (size_t)d * 6;
      const double x1 = (double)p[0] * fx, y1 = (double)p[1] * fy, x2 = (double)p[2] * fx, y2 = (double)p[3] * fy;
      sm.dbox[d][0] = x1; sm.dbox[d][1] = y1; sm.dbox[d][2] = x2; sm.dbox[d][3] = y2;
      sm.darea[d] = (x2 - x1) * (y2 - y1);
      score = p[4];
    }
    rec_score[cell * MAX_DET + d] = score;
  }
  __syncthreads();
  for (int i = tid; i < nd * ng; i += 256) {
    const int d = i / ng, g = i - d * ng;
    const double ax2 = sm.dbox[d][2], bx2 = sm.gbox[g][2], ax1 = sm.dbox[d][0], bx1 = sm.gbox[g][0];
    const double ay2 = sm.dbox[d][3], by2 = sm.gbox[g][3], ay1 = sm.dbox[d][1], by1 = sm.gbox[g][1];
    const double iw = (bx2 < ax2 ? bx2 : ax2) - (bx1 > ax1 ? bx1 : ax1);
    const double ih = (by2 < ay2 ? by2 : ay2) - (by1 > ay1 ? by1 : ay1);
    double v = 0.0;
    if (!(iw <= 0.0) && !(ih <= 0.0)) {
      const double in = iw * ih;
      const double un = sm.darea[d] + sm.garea[g] - in;
      v = in / un;
    }
    sm.iou[i] = v;
  }
  // ---- per area range: the stable sort by the ignore flag, and the count of non-ignored ground truths
  if (tid < NAREA) {
    const double lo = area_rngs[2 * tid], hi = area_rngs[2 * tid + 1];
    int n = 0;
    for (int g = 0; g < ng; ++g)
      if (!(sm.garea[g] < lo || sm.garea[g] > hi)) sm.order[tid][n++] = (unsigned char)g;
    sm.nnon[tid] = n;
    rec_ngt[cell * NAREA + tid] = n;
    for (int g = 0; g < ng; ++g)
      if (sm.garea[g] < lo || sm.garea[g] > hi) sm.order[tid][n++] = (unsigned char)g;
  }
  __syncthreads();
  if (tid >= 64) return;

  // ---- wave 0: lane a * 10 + t walks the detections in score order
  const bool live = tid < NPAIR;
  const int a = live ? tid / NTHR : 0, t = live ? tid % NTHR : 0;
  const double lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
  const double cap = 1.0 - 1e-10;
  const double thr0 = cap < iou_thrs[t] ? cap : iou_thrs[t];
  const int nnon = sm.nnon[a];
  unsigned long long taken = 0ull;
  for (int d = 0; d < MAX_DET; ++d) {
    bool dm = false, ig = false;
    if (live && d < nd) {
      double thr = thr0;
      int m = -1;
      bool m_ig = false;
      for (int k = 0; k < ng; ++k) {
        const int g = sm.order[a][k];
        const bool g_ig = k >= nnon;
        if ((taken >> g) & 1ull) continue;
        if (m > -1 && !m_ig && g_ig) break;
        const double v = sm.iou[d * ng + g];
        if (v < thr) continue;
        thr = v;
        m = g;
        m_ig = g_ig;
      }
      if (m > -1) {
        dm = true;
        ig = m_ig;
        taken |= 1ull << m;
      } else {
        const double ad = sm.darea[d];
        ig = ad < lo || ad > hi;
      }
    }
    const unsigned long long wm = __ballot(dm), wi = __ballot(ig);
    if (tid == 0) {
      rec_dtm[cell * MAX_DET + d] = wm;
      rec_dtig[cell * MAX_DET + d] = wi;
    }
  }
}

inline bool misaligned(const void* p, size_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" int t3d_ssd_cap_per_image(const float* out, const int* counts, int B, int num_classes, int max_per_class,
                                     int max_per_img, int* counts_out, void* stream) {
  if (!out || !counts || !counts_out || misaligned(out, 4) || misaligned(counts, 4) || misaligned(counts_out, 4)) return T3D_ERR_ARG;
  if (B < 0 || num_classes < 1 || max_per_class < 1 || max_per_img < 0) return T3D_ERR_ARG;
  if ((long long)num_classes * max_per_class > CAP_MAX_ROWS) return T3D_ERR_UNSUPPORTED;
  if (B == 0) return T3D_OK;
  T3D_LAUNCH(ssd_cap_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out, counts, num_classes, max_per_class,
             max_per_img, counts_out);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_coco_match(const float* out, const int* counts, int B, int num_classes, int max_per_class,
                              const float* gt_boxes, const int* gt_labels, const int* gt_counts, int G, const int* ori_shapes,
                              int in_w, int in_h, const double* iou_thrs, const double* area_rngs, int base, int R,
                              float* rec_score, unsigned long long* rec_dtm, unsigned long long* rec_dtig, int* rec_ndt,
                              int* rec_ngt, int* rec_valid, void* stream) {
  if (!out || !counts || !gt_counts || !ori_shapes || !iou_thrs || !area_rngs || !rec_score || !rec_dtm || !rec_dtig || !rec_ndt ||
      !rec_ngt || !rec_valid)
    return T3D_ERR_ARG;
  if (G < 0 || (G > 0 && (!gt_boxes || !gt_labels))) return T3D_ERR_ARG;
  if (misaligned(out, 4) || misaligned(counts, 4) || misaligned(gt_boxes, 4) || misaligned(gt_labels, 4) || misaligned(gt_counts, 4) ||
      misaligned(ori_shapes, 4) || misaligned(iou_thrs, 8) || misaligned(area_rngs, 8) || misaligned(rec_score, 4) ||
      misaligned(rec_dtm, 8) || misaligned(rec_dtig, 8) || misaligned(rec_ndt, 4) || misaligned(rec_ngt, 4) || misaligned(rec_valid, 4))
    return T3D_ERR_ARG;
  if (B < 0 || num_classes < 1 || max_per_class < 1 || in_w <= 0 || in_h <= 0 || base < 0 || R < 0 || (long long)base + B > R ||
      (long long)B * num_classes > 0x7fffffffLL)
    return T3D_ERR_ARG;
  if (G > MAX_GT) return T3D_ERR_UNSUPPORTED;
  if (B == 0) return T3D_OK;
  T3D_LAUNCH(coco_match_kernel, dim3(B * num_classes), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), out, counts, num_classes,
             max_per_class, gt_boxes, gt_labels, gt_counts, G, ori_shapes, in_w, in_h, iou_thrs, area_rngs, base, rec_score, rec_dtm,
             rec_dtig, rec_ndt, rec_ngt, rec_valid);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
