// The Objectron evaluation protocol on the device (the reference's final report, scripts/objectron_eval.py:116-175, which
// drives objectron.dataset.eval.Evaluator): per frame every predicted box is matched to an annotated instance, lifted
// (lift_2d, portrait), rescaled with the ground plane and measured against the metric-scale ground truth -- 2-D pixel
// error, azimuth / polar viewpoint error, 3-D IoU, ADD, ADD-S -- and the per-frame hit / miss counts at 21 thresholds per
// metric go into the evaluator's record, from which the host computes average precision once at the end.
//
// PARITY UNPINNED: objectron.dataset.eval / objectron.dataset.metrics come from the git submodule 3rdparty/Objectron, an
// EMPTY directory in the reference.  The protocol implemented here is the one DESIGN.md section 7
// states ("Objectron evaluation protocol"), restated from the reference's own script and the published evaluator; that
// statement is the definition, tests/objectron_eval_ref.py is its plain-loop numpy form.
// Stated deviation: a non-finite intermediate (a zero dot product in the scale, a singular viewpoint system) does not trap:
// the non-finite metric is carried as it is, misses every threshold and is left out of the running sums.
//
//   t3d_objectron_pairs    one 128-thread workgroup per (frame, prediction slot), like iou3d_kernel:
//     all      match: lane i owns instances i, i + 128, ...: ||pred[1:9] - kp2d_i[1:9]||_F, first minimum wins
//     wave 0   lift of the prediction (lift_wave, default NDC camera)
//     wave 1   meanwhile: the matched instance's kp3d into LDS, pixel error, the instance's viewpoint
//     wave 0   scale (sort of 8 dot products), the prediction's viewpoint (4 x 4 pivoted solve), ADD / ADD-S over lanes,
//              box-box IoU (box_iou_wave: fit both, clip the 12 faces over lanes)
//   t3d_objectron_hitmiss  one workgroup per frame: instance count, a thread per (metric, threshold) walking the frame's
//     predictions in slot order, one thread for the partial sums; plain stores into row base + f, no atomics in memory.
#include "box_geometry.h"

namespace {

constexpr double VIS = 0.1, MAX_PIXEL = 0.1, MAX_AZIMUTH = 30.0, MAX_POLAR = 20.0, MAX_DIST = 1.0;
constexpr int NBINS = 21, NMETRICS = 6, M_IOU = 3;        // per-slot order: pixel, azimuth, polar, iou, add, adds
constexpr double RAD2DEG = 57.29577951308232;             // 180 / pi, as numpy.degrees multiplies

struct EvalSmem {
  double A[12 * LD];
  double V[12 * LD];
  double vert[2][9][3];          // 0: the lifted prediction, 1: the matched instance's kp3d
  double poly[12][2][MAXV][3];
  double pk[18];                 // the prediction, normalised
  double bd[128];
  int bi[128];
  double gview[2], pixel, scale;
  int match;
};

__device__ __forceinline__ double dist3(const double* a, const double* b) {
  const double x = a[0] - b[0], y = a[1] - b[1], z = a[2] - b[2];
  return sqrt(x * x + y * y + z * z);
}

// Viewpoint of a 9 x 3 box V (one thread): with O = the unit box scaled by V's edge lengths and homogeneous 4 x 9 matrices
// Oh, Vh, T = Oh Vh^T (Vh Vh^T)^-1 and (x, y, z) = T[0:3, 3].  Only that column is needed: y = (Vh Vh^T)^-1 e_3 by Gaussian
// elimination with partial pivoting, then T[r][3] = sum_k O[k][r] (Vh[:, k] . y).  A zero pivot divides: inf / nan, carried.
__device__ void viewpoint(const double (*v)[3], double& azimuth, double& polar) {
  const double size[3] = {dist3(v[5], v[1]), dist3(v[3], v[1]), dist3(v[2], v[1])};
  double s[4][5];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 5; ++j) s[i][j] = 0.0;
  for (int k = 0; k < 9; ++k) {
    const double h[4] = {v[k][0], v[k][1], v[k][2], 1.0};
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < 4; ++j) s[i][j] += h[i] * h[j];
  }
  s[3][4] = 1.0;
  for (int c = 0; c < 4; ++c) {
    int piv = c;
    for (int r = c + 1; r < 4; ++r)
      if (fabs(s[r][c]) > fabs(s[piv][c])) piv = r;
    for (int j = 0; j < 5; ++j) {
      const double a = s[c][j], b = s[piv][j];
      s[c][j] = b;
      s[piv][j] = a;
    }
    for (int r = c + 1; r < 4; ++r) {
      const double m = s[r][c] / s[c][c];
      for (int j = c; j < 5; ++j) s[r][j] -= m * s[c][j];
    }
  }
  double y[4];
  for (int c = 3; c >= 0; --c) {
    double a = s[c][4];
    for (int j = c + 1; j < 4; ++j) a -= s[c][j] * y[j];
    y[c] = a / s[c][c];
  }
  double t[3] = {0.0, 0.0, 0.0};
  for (int k = 1; k < 9; ++k) {          // (O[0] is the origin)
    const double w = v[k][0] * y[0] + v[k][1] * y[1] + v[k][2] * y[2] + y[3];
    for (int r = 0; r < 3; ++r) t[r] += 0.5 * c_sign[k - 1][r] * size[r] * w;
  }
  azimuth = atan2(t[2], t[0]) * RAD2DEG;
  polar = atan2(t[1], hypot(t[0], t[2])) * RAD2DEG;
}

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

__global__ __launch_bounds__(128) void objectron_pairs_kernel(const double* __restrict__ pred, const int* __restrict__ pred_count,
                                                              const double* __restrict__ gt2, const double* __restrict__ gt3,
                                                              const double* __restrict__ vis, const int* __restrict__ gt_count,
                                                              const double* __restrict__ planes, int P, int G, double sx, double sy,
                                                              double* __restrict__ metrics, int* __restrict__ matched) {
  __shared__ EvalSmem sm;
  const int f = blockIdx.x / P, p = blockIdx.x % P, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (p >= clampi(pred_count[f], P)) return;          // slots past the count are never read
  const int ng = clampi(gt_count[f], G);
  const size_t slot = (size_t)f * P + p;
  if (tid < 18) sm.pk[tid] = pred[slot * 18 + tid] * ((tid & 1) ? sy : sx);
  __syncthreads();

  // ---- match: argmin of the Frobenius distance over the 8 corner keypoints; a nan distance sorts first, as numpy.argmin has it
  double best = 0.0;
  int bi = -1;
  for (int i = tid; i < ng; i += 128) {
    const double* g = gt2 + ((size_t)f * G + i) * 18;
    double s = 0.0;
    for (int k = 2; k < 18; ++k) {
      const double d = sm.pk[k] - g[k];
      s += d * d;
    }
    double d = sqrt(s);
    if (d != d) d = -INFINITY;
    if (bi < 0 || d < best) { best = d; bi = i; }
  }
  sm.bd[tid] = best;
  sm.bi[tid] = bi;
  __syncthreads();
  if (tid == 0) {
    for (int t = 1; t < 128 && t < ng; ++t) {
      const double d = sm.bd[t];
      const int i = sm.bi[t];
      if (d < best || (d == best && i < bi)) { best = d; bi = i; }
    }
    if (bi >= 0 && vis[(size_t)f * G + bi] < VIS) bi = -1;
    sm.match = bi;
  }
  __syncthreads();
  const int m = sm.match;
  double* out = metrics + slot * NMETRICS;
  if (m < 0) {
    if (tid == 0) {
      out[0] = MAX_PIXEL; out[1] = MAX_AZIMUTH; out[2] = MAX_POLAR; out[3] = 0.0; out[4] = MAX_DIST; out[5] = MAX_DIST;
      matched[slot] = -1;
    }
    return;
  }

  if (wave == 0) {
    lift_wave<double>(sm.pk, 1, 2.0, 2.0, 0.0, 0.0, sm.A, sm.V, sm.vert[0], lane);
  } else {
    if (lane < 27) sm.vert[1][lane / 3][lane % 3] = gt3[((size_t)f * G + m) * 27 + lane];
    wave_sync();
    if (lane == 0) {
      const double* g = gt2 + ((size_t)f * G + m) * 18;
      double s = 0.0;
      for (int k = 1; k < 9; ++k) {
        const double dx = sm.pk[2 * k] - g[2 * k], dy = sm.pk[2 * k + 1] - g[2 * k + 1];
        s += sqrt(dx * dx + dy * dy);
      }
      sm.pixel = s / 8.0;
    } else if (lane == 1) {
      viewpoint(sm.vert[1], sm.gview[0], sm.gview[1]);
    }
  }
  __syncthreads();
  if (wave != 0) return;

  // ---- scale from the ground plane: mean over the 4 smallest of the 8 corner dot products
  if (lane == 0) {
    const double* pl = planes + (size_t)f * 6;
    double d[8];
    for (int k = 0; k < 8; ++k) d[k] = sm.vert[0][k + 1][0] * pl[3] + sm.vert[0][k + 1][1] * pl[4] + sm.vert[0][k + 1][2] * pl[5];
    for (int i = 1; i < 8; ++i) {
      const double x = d[i];
      int j = i - 1;
      while (j >= 0 && (d[j] > x || (d[j] != d[j] && x == x))) { d[j + 1] = d[j]; --j; }     // nan last, as numpy.sort has it
      d[j + 1] = x;
    }
    const double cn = pl[0] * pl[3] + pl[1] * pl[4] + pl[2] * pl[5];
    sm.scale = (cn / d[0] + cn / d[1] + cn / d[2] + cn / d[3]) / 4.0;
  }
  wave_sync();
  if (lane < 27) sm.vert[0][lane / 3][lane % 3] *= sm.scale;
  wave_sync();

  double add = 0.0, adds = 0.0;
  if (lane < 9) {
    add = dist3(sm.vert[0][lane], sm.vert[1][lane]);
    bool isnan_ = false;
    for (int j = 0; j < 9; ++j) {
      const double d = dist3(sm.vert[0][lane], sm.vert[1][j]);
      isnan_ = isnan_ || d != d;
      if (j == 0 || d < adds) adds = d;
    }
    if (isnan_) adds = NAN;               // numpy.min propagates
  }
  add = wave_sum_d(add) / 9.0;
  adds = wave_sum_d(adds) / 9.0;
  double az_err = 0.0, polar_err = 0.0;
  if (lane == 0) {
    double az, po;
    viewpoint(sm.vert[0], az, po);
    polar_err = fabs(po - sm.gview[1]);
    az_err = fabs(az - sm.gview[0]);
    if (az_err > 180.0) az_err = 360.0 - az_err;
  }
  const double iou = box_iou_wave(sm.vert[0], sm.vert[1], sm.poly, lane);
  if (lane == 0) {
    out[0] = sm.pixel; out[1] = az_err; out[2] = polar_err; out[3] = iou; out[4] = add; out[5] = adds;
    matched[slot] = m;
  }
}

__global__ __launch_bounds__(128) void objectron_hitmiss_kernel(const double* __restrict__ metrics, const int* __restrict__ matched,
                                                                const int* __restrict__ pred_count, const double* __restrict__ gt2,
                                                                const double* __restrict__ gt3, const double* __restrict__ vis,
                                                                const int* __restrict__ gt_count, const double* __restrict__ thr,
                                                                int P, int G, int base, int* __restrict__ valid,
                                                                int* __restrict__ ninst, int* __restrict__ hit,
                                                                int* __restrict__ miss, double* __restrict__ sums) {
  __shared__ int s_vis[128];
  const int f = blockIdx.x, tid = threadIdx.x;
  const int np = clampi(pred_count[f], P), ng = clampi(gt_count[f], G);
  // instances that count: visible, centre keypoint strictly inside the frame, in front of the camera
  int n = 0;
  for (int i = tid; i < ng; i += 128) {
    const size_t gi = (size_t)f * G + i;
    const double cx = gt2[gi * 18], cy = gt2[gi * 18 + 1];
    n += vis[gi] > VIS && cx > 0.0 && cx < 1.0 && cy > 0.0 && cy < 1.0 && gt3[gi * 27 + 2] < 0.0;
  }
  s_vis[tid] = n;
  __syncthreads();
  n = 0;
  for (int t = 0; t < 128; ++t) n += s_vis[t];
  const bool ok = n > 0;
  const size_t row = (size_t)base + f;
  if (tid == 0) {
    valid[row] = ok;
    ninst[row] = ng;
  }
  if (tid < NMETRICS * NBINS) {
    const int m = tid / NBINS;
    const double t = thr[tid];
    int h = 0, ms = 0;
    if (ok) {
      for (int p = 0; p < np; ++p) {
        const double v = metrics[((size_t)f * P + p) * NMETRICS + m];
        const bool hp = (m == M_IOU) ? v >= t : v <= t;
        h += hp;
        ms += !hp;
      }
    }
    hit[row * (NMETRICS * NBINS) + tid] = h;
    miss[row * (NMETRICS * NBINS) + tid] = ms;
  } else if (tid == NMETRICS * NBINS) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};      // error_2d, iou_3d, azimuth, polar, matched
    if (ok) {
      for (int p = 0; p < np; ++p) {
        const size_t slot = (size_t)f * P + p;
        if (matched[slot] < 0) continue;
        const double* v = metrics + slot * NMETRICS;
        if (isfinite(v[0])) s[0] += v[0];
        if (isfinite(v[3])) s[1] += v[3];
        if (isfinite(v[1])) s[2] += v[1];
        if (isfinite(v[2])) s[3] += v[2];
        s[4] += 1.0;
      }
    }
    for (int i = 0; i < 5; ++i) sums[row * 5 + i] = s[i];
  }
}

}  // namespace

extern "C" int t3d_objectron_pairs(const double* pred_kp, const int* pred_count, const double* gt_kp2d, const double* gt_kp3d,
                                   const double* gt_visibility, const int* gt_count, const double* planes, int F, int P, int G,
                                   double sx, double sy, double* metrics, int* matched, void* stream) {
  if (!pred_kp || !pred_count || !gt_kp2d || !gt_kp3d || !gt_visibility || !gt_count || !planes || !metrics || !matched)
    return T3D_ERR_ARG;
  if (F <= 0 || P <= 0 || G <= 0 || (long long)F * P > 0x7fffffffLL) return T3D_ERR_ARG;
  T3D_LAUNCH(objectron_pairs_kernel, dim3(F * P), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), pred_kp, pred_count,
             gt_kp2d, gt_kp3d, gt_visibility, gt_count, planes, P, G, sx, sy, metrics, matched);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_objectron_hitmiss(const double* metrics, const int* matched, const int* pred_count, const double* gt_kp2d,
                                     const double* gt_kp3d, const double* gt_visibility, const int* gt_count,
                                     const double* thresholds, int F, int P, int G, int base, int capacity, int* valid,
                                     int* num_instances, int* hit, int* miss, double* sums, void* stream) {
  if (!metrics || !matched || !pred_count || !gt_kp2d || !gt_kp3d || !gt_visibility || !gt_count || !thresholds || !valid ||
      !num_instances || !hit || !miss || !sums)
    return T3D_ERR_ARG;
  if (F <= 0 || P <= 0 || G <= 0 || base < 0 || capacity <= 0 || (long long)base + F > capacity) return T3D_ERR_ARG;
  T3D_LAUNCH(objectron_hitmiss_kernel, dim3(F), dim3(128), 0, reinterpret_cast<hipStream_t>(stream), metrics, matched,
             pred_count, gt_kp2d, gt_kp3d, gt_visibility, gt_count, thresholds, P, G, base, valid, num_instances, hit, miss, sums);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
