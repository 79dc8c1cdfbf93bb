// MultiBox training loss of the SSD detector and its gradients with respect to the head outputs (the training half of
// configs/detection/mnv2_ssd_300_2_heads.py:41-55 of the reference: MaxIoUAssigner(pos_iou_thr = neg_iou_thr = 0.4,
// min_pos_iou = 0, gt_max_assign_all = False), smoothl1_beta = 1, neg_pos_ratio = 3) in TWO launches with nothing read back:
//   mb_image_kernel   one workgroup per image: IoU of every (ground truth, anchor) pair, the assignment, the per-anchor
//                     cross-entropy, hard-negative mining (a radix select on the fp32 bit pattern, ties by anchor index)
//                     and the image's two fp64 partial sums -- the per-anchor state lives in LDS;
//   mb_grad_kernel    a grid over B x A: forms avg = max(sum_b num_pos[b], 1), writes the gradients (pads included) and,
//                     in workgroup 0, the four scalars.
// The implementing mmdetection fork is external to the reference; the arithmetic restates the published mmdet 2.x
// SSDHead.loss / MaxIoUAssigner / DeltaXYWHBBoxCoder / smooth_l1_loss (tests/ssd_loss_ref.py is the definition) -- parity
// with the reference's detector is unpinned, as for csrc/ssd.hip.  The config's loss_balancing is not built (no published
// definition).
// Determinism: no floating-point atomics.  The IoU is computed with every operation rounded on its own, so every decision
// (assignment, ties) is exact against a float32 restatement; the fp64 sums run over a fixed tree (a thread adds its
// anchors in ascending order, the lanes and waves are combined in a fixed order, the images in index order).
#include "common.h"

namespace {

constexpr int kMaxG = 64;        // ground-truth slots per image the LDS plan holds
constexpr int kMaxA = 16384;     // anchors per image the LDS plan holds (8 bytes each)
constexpr int kNT = 512, kNW = kNT / 64;
constexpr int kFixedLds = kMaxG * 8 + 2 * kNW * 8 + kMaxG * 5 * 4 + kMaxG * 4 + 256 * 4 + 16 * 4;
static_assert(kFixedLds % 16 == 0, "the per-anchor arrays start 16-byte aligned");
static_assert(kFixedLds + 8 * kMaxA <= 160 * 1024, "LDS plan");

struct MbLevel {
  const void *cls, *reg;   // [B*HW][cls_stride], [B*HW][reg_stride] (storage dtype)
  float *dcls, *dreg;      // the same rows in fp32, or null
  int HW, A, cls_stride, reg_stride;
};

struct MbArgs {
  MbLevel lv[2];
  int nlevels, dtype;
  const float* anchors;    // [Atot][4]
  const float* gt_boxes;   // [B][G][4]
  const int* gt_labels;    // [B][G]
  const int* gt_counts;    // [B]
  int B, G, Atot, nc, ratio, grads;
  float pos_thr, min_pos, beta, sx, sy, sw, sh;
  double* partial;         // [B][2]: the image's sums of ce and of smooth L1
  double* scalars;         // [4]
  int* num_pos;            // [B]
  int* assigned;           // [B][Atot]
};

__device__ __forceinline__ float ldval(const void* p, size_t i, int dtype) {
  return dtype == T3D_F32 ? reinterpret_cast<const float*>(p)[i] : (float)reinterpret_cast<const bf16_t*>(p)[i];
}

// anchor i of image b -> its level's pointers and the offsets of its class / box channels
struct MbLoc {
  const void *cls, *reg;
  float *dcls, *dreg;
  size_t row, cb, rb;
  int an, A, cls_stride, reg_stride;
};
__device__ __forceinline__ MbLoc locate(const MbArgs& a, int b, int i) {
  const int n0 = a.lv[0].HW * a.lv[0].A;
  const bool up = a.nlevels > 1 && i >= n0;
  MbLoc o;
  o.cls = up ? a.lv[1].cls : a.lv[0].cls;
  o.reg = up ? a.lv[1].reg : a.lv[0].reg;
  o.dcls = up ? a.lv[1].dcls : a.lv[0].dcls;
  o.dreg = up ? a.lv[1].dreg : a.lv[0].dreg;
  o.A = up ? a.lv[1].A : a.lv[0].A;
  o.cls_stride = up ? a.lv[1].cls_stride : a.lv[0].cls_stride;
  o.reg_stride = up ? a.lv[1].reg_stride : a.lv[0].reg_stride;
  const int HW = up ? a.lv[1].HW : a.lv[0].HW;
  const int j = up ? i - n0 : i;
  const int px = j / o.A;
  o.an = j - px * o.A;
  o.row = (size_t)b * HW + px;
  o.cb = o.row * o.cls_stride + (size_t)o.an * (a.nc + 1);
  o.rb = o.row * o.reg_stride + (size_t)o.an * 4;
  return o;
}

// every operation rounded on its own (no contraction): the float32 restatement reproduces it bit for bit
__device__ __forceinline__ float box_area(float x1, float y1, float x2, float y2) {
  return __fmul_rn(__fsub_rn(x2, x1), __fsub_rn(y2, y1));
}
__device__ __forceinline__ float iou_rn(float gx1, float gy1, float gx2, float gy2, float garea, float ax1, float ay1,
                                        float ax2, float ay2, float aarea) {
  const float iw = fmaxf(__fsub_rn(fminf(gx2, ax2), fmaxf(gx1, ax1)), 0.f);
  const float ih = fmaxf(__fsub_rn(fminf(gy2, ay2), fmaxf(gy1, ay1)), 0.f);
  const float inter = __fmul_rn(iw, ih);
  const float uni = fmaxf(__fsub_rn(__fadd_rn(garea, aarea), inter), 1e-6f);
  return __fdiv_rn(inter, uni);
}

// cross-entropy of one anchor's nc + 1 logits against `label`
__device__ __forceinline__ float anchor_ce(const void* cls, size_t cb, int nc, int label, int dtype) {
  float mx = ldval(cls, cb, dtype);
  for (int k = 1; k <= nc; ++k) mx = fmaxf(mx, ldval(cls, cb + k, dtype));
  float den = 0.f;
  for (int k = 0; k <= nc; ++k) den += expf(ldval(cls, cb + k, dtype) - mx);
  return logf(den) - (ldval(cls, cb + label, dtype) - mx);
}

// DeltaXYWH target of ground truth g for anchor an, divided by the stds
__device__ __forceinline__ void box_target(const float* an, const float* g, const MbArgs& a, float t[4]) {
  const float px = (an[0] + an[2]) * 0.5f, py = (an[1] + an[3]) * 0.5f, pw = an[2] - an[0], ph = an[3] - an[1];
  const float gx = (g[0] + g[2]) * 0.5f, gy = (g[1] + g[3]) * 0.5f, gw = g[2] - g[0], gh = g[3] - g[1];
  t[0] = ((gx - px) / pw) / a.sx;
  t[1] = ((gy - py) / ph) / a.sy;
  t[2] = logf(gw / pw) / a.sw;
  t[3] = logf(gh / ph) / a.sh;
}
__device__ __forceinline__ float smooth_l1(float diff, float beta) {
  const float d = fabsf(diff);
  return d < beta ? 0.5f * d * d / beta : d - 0.5f * beta;
}
__device__ __forceinline__ float smooth_l1_grad(float diff, float beta) {
  const float d = fabsf(diff);
  return d < beta ? diff / beta : (diff > 0.f ? 1.f : -1.f);
}

__global__ __launch_bounds__(kNT) void mb_image_kernel(const MbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* gkey = reinterpret_cast<unsigned long long*>(smem);   // [kMaxG] (best IoU bits << 32) | ~anchor
  double* red = reinterpret_cast<double*>(gkey + kMaxG);                    // [2][kNW]
  float* gbox = reinterpret_cast<float*>(red + 2 * kNW);                    // [kMaxG][5] x1, y1, x2, y2, area
  int* glab = reinterpret_cast<int*>(gbox + kMaxG * 5);                     // [kMaxG] label, -1: slot skipped
  int* hist = glab + kMaxG;                                                 // [256]
  int* misc = hist + 256;                                                   // [16]
  float* mval = reinterpret_cast<float*>(misc + 16);                        // [A] best IoU, then the ce (its bit pattern is the mining key)
  int* asg = reinterpret_cast<int*>(mval + a.Atot);                         // [A]
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, A = a.Atot;
  int count = a.gt_counts[b];
  count = count < 0 ? 0 : (count > a.G ? a.G : count);

  // ---- valid ground truth
  if (tid < kMaxG) {
    int lab = -1;
    if (tid < count) {
      const float* g = a.gt_boxes + ((size_t)b * a.G + tid) * 4;
      const float x1 = g[0], y1 = g[1], x2 = g[2], y2 = g[3];
      const int l = a.gt_labels[(size_t)b * a.G + tid];
      const bool fin = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2);
      if (fin && x2 > x1 && y2 > y1 && l >= 0 && l < a.nc) lab = l;
      gbox[tid * 5] = x1; gbox[tid * 5 + 1] = y1; gbox[tid * 5 + 2] = x2; gbox[tid * 5 + 3] = y2;
      gbox[tid * 5 + 4] = box_area(x1, y1, x2, y2);
    }
    glab[tid] = lab;
    gkey[tid] = 0ull;
  }
  if (tid < 16) misc[tid] = 0;
  for (int i = tid; i < A; i += kNT) { mval[i] = -1.f; asg[i] = -1; }
  __syncthreads();

  // ---- IoU: per anchor the best ground truth (first on ties), per ground truth the best anchor (lowest on ties)
  for (int i = 0; i < count; ++i) {
    if (glab[i] < 0) continue;
    const float gx1 = gbox[i * 5], gy1 = gbox[i * 5 + 1], gx2 = gbox[i * 5 + 2], gy2 = gbox[i * 5 + 3], ga = gbox[i * 5 + 4];
    unsigned long long best = 0ull;
    for (int j = tid; j < A; j += kNT) {
      const float ax1 = a.anchors[4 * j], ay1 = a.anchors[4 * j + 1], ax2 = a.anchors[4 * j + 2], ay2 = a.anchors[4 * j + 3];
      const float v = iou_rn(gx1, gy1, gx2, gy2, ga, ax1, ay1, ax2, ay2, box_area(ax1, ay1, ax2, ay2));
      if (v > mval[j]) { mval[j] = v; asg[j] = i; }
      const unsigned long long key = ((unsigned long long)(v > 0.f ? __float_as_uint(v) : 0u) << 32) | (0xffffffffu - (unsigned)j);
      best = key > best ? key : best;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o > best ? o : best;
    }
    if (lane == 0 && best) atomicMax(&gkey[i], best);
  }
  __syncthreads();
  for (int j = tid; j < A; j += kNT)
    if (!(mval[j] >= a.pos_thr)) asg[j] = -1;
  __syncthreads();
  if (tid == 0) {
    for (int i = 0; i < count; ++i) {           // ascending: a later ground truth overrides an earlier one
      if (glab[i] < 0) continue;
      const unsigned long long key = gkey[i];
      const unsigned lo = (unsigned)key;
      if (!lo) continue;
      const unsigned j = 0xffffffffu - lo;
      if (__uint_as_float((unsigned)(key >> 32)) >= a.min_pos && j < (unsigned)A) asg[j] = i;
    }
  }
  __syncthreads();

  // ---- cross-entropy of every anchor against its label; the positives are counted
  int mypos = 0;
  for (int j = tid; j < A; j += kNT) {
    const int s = asg[j];
    const MbLoc L = locate(a, b, j);
    mval[j] = anchor_ce(L.cls, L.cb, a.nc, s >= 0 ? glab[s] : a.nc, a.dtype);
    mypos += s >= 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) mypos += __shfl_xor(mypos, off, 64);
  if (lane == 0 && mypos) atomicAdd(&misc[0], mypos);
  __syncthreads();
  const int npos = misc[0];
  const long long want = (long long)a.ratio * npos;
  const int k = (int)(want < (long long)(A - npos) ? want : (long long)(A - npos));

  // ---- hard-negative mining: the k negatives that come first by (ce descending, anchor ascending)
  if (k > 0) {
    // radix select, 8 bits a pass from the top: the k-th largest key T and how many of the keys equal to T are taken
    unsigned prefix = 0u;
    int rem = k;
    for (int shift = 24; shift >= 0; shift -= 8) {
      if (tid < 256) hist[tid] = 0;
      __syncthreads();
      for (int j = tid; j < A; j += kNT) {
        const unsigned key = __float_as_uint(mval[j]);
        if (asg[j] == -1 && (shift == 24 || (key >> (shift + 8)) == (prefix >> (shift + 8)))) atomicAdd(&hist[(key >> shift) & 255u], 1);
      }
      __syncthreads();
      if (wv == 0) {                            // lane l holds bins 255 - 4 l .. 252 - 4 l, scanned from the top bin down
        int c[4], s = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) { c[q] = hist[255 - 4 * lane - q]; s += c[q]; }
        int incl = s;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
          const int o = __shfl_up(incl, off, 64);
          if (lane >= off) incl += o;
        }
        int excl = incl - s;
        if (excl < rem && rem <= incl) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            if (excl < rem && rem <= excl + c[q]) { misc[1] = 255 - 4 * lane - q; misc[2] = rem - excl; }
            excl += c[q];
          }
        }
      }
      __syncthreads();
      prefix |= (unsigned)misc[1] << shift;
      rem = misc[2];
      __syncthreads();
    }
    // keys above T are mined; of the keys equal to T the first `rem` in anchor order (chunks of kNT anchors in thread order)
    int running = 0;
    for (int base = 0; base < A; base += kNT) {
      const int j = base + tid;
      bool tie = false;
      if (j < A && asg[j] == -1) {
        const unsigned key = __float_as_uint(mval[j]);
        if (key > prefix) asg[j] = -2;
        tie = key == prefix;
      }
      if (running < rem) {                      // (uniform)
        const unsigned long long m = __ballot(tie);
        if (lane == 0) misc[4 + wv] = __popcll(m);
        __syncthreads();
        int before = running, total = running;
#pragma unroll
        for (int w = 0; w < kNW; ++w) { const int n = misc[4 + w]; before += w < wv ? n : 0; total += n; }
        const int rank = before + __popcll(m & ((1ull << lane) - 1ull));
        if (tie && rank < rem) asg[j] = -2;
        running = total;
        __syncthreads();
      }
    }
  }
  __syncthreads();

  // ---- the image's sums (fp64) and outputs
  double lc = 0.0, lb = 0.0;
  for (int j = tid; j < A; j += kNT) {
    const int s = asg[j];
    a.assigned[(size_t)b * A + j] = s;
    if (s == -1) continue;
    lc += (double)mval[j];
    if (s >= 0) {
      const MbLoc L = locate(a, b, j);
      float t[4];
      box_target(a.anchors + 4 * (size_t)j, gbox + s * 5, a, t);
#pragma unroll
      for (int q = 0; q < 4; ++q) lb += (double)smooth_l1(ldval(L.reg, L.rb + q, a.dtype) - t[q], a.beta);
    }
  }
  lc = wave_sum_d(lc);
  lb = wave_sum_d(lb);
  if (lane == 0) { red[wv] = lc; red[kNW + wv] = lb; }
  __syncthreads();
  if (tid == 0) {
    double sc = 0.0, sb = 0.0;
#pragma unroll
    for (int w = 0; w < kNW; ++w) { sc += red[w]; sb += red[kNW + w]; }
    a.partial[2 * (size_t)b] = sc;
    a.partial[2 * (size_t)b + 1] = sb;
    a.num_pos[b] = npos;
  }
}

__global__ __launch_bounds__(256) void mb_grad_kernel(const MbArgs a) {
  __shared__ int tot_s;
  const int tid = threadIdx.x, A = a.Atot;
  if (tid == 0) tot_s = 0;
  __syncthreads();
  int mine = 0;
  for (int i = tid; i < a.B; i += 256) mine += a.num_pos[i];
  if (mine) atomicAdd(&tot_s, mine);            // (integers: the order does not matter)
  __syncthreads();
  const int tot = tot_s;
  const int avg_i = tot > 1 ? tot : 1;
  if (blockIdx.x == 0 && tid == 0) {
    double sc = 0.0, sb = 0.0, mined = 0.0;
    for (int i = 0; i < a.B; ++i) {             // image order
      sc += a.partial[2 * (size_t)i];
      sb += a.partial[2 * (size_t)i + 1];
      const int np = a.num_pos[i];
      const long long want = (long long)a.ratio * np;
      mined += (double)(want < (long long)(A - np) ? want : (long long)(A - np));
    }
    a.scalars[0] = sc / (double)avg_i;
    a.scalars[1] = sb / (double)avg_i;
    a.scalars[2] = (double)tot;
    a.scalars[3] = mined;
  }
  if (!a.grads) return;
  const long long idx = (long long)blockIdx.x * 256 + tid;
  if (idx >= (long long)a.B * A) return;
  const int b = (int)(idx / A), j = (int)(idx - (long long)b * A);
  const float avg = (float)avg_i;
  const int s = a.assigned[idx];
  const MbLoc L = locate(a, b, j);
  float* dc = L.dcls + L.cb;
  float* dr = L.dreg + L.rb;
  if (s == -1) {
    for (int k = 0; k <= a.nc; ++k) dc[k] = 0.f;
  } else {
    const int label = s >= 0 ? a.gt_labels[(size_t)b * a.G + s] : a.nc;
    float mx = ldval(L.cls, L.cb, a.dtype);
    for (int k = 1; k <= a.nc; ++k) mx = fmaxf(mx, ldval(L.cls, L.cb + k, a.dtype));
    float den = 0.f;
    for (int k = 0; k <= a.nc; ++k) den += expf(ldval(L.cls, L.cb + k, a.dtype) - mx);
    for (int k = 0; k <= a.nc; ++k) {
      const float p = expf(ldval(L.cls, L.cb + k, a.dtype) - mx) / den;
      dc[k] = (p - (k == label ? 1.f : 0.f)) / avg;
    }
  }
  if (s >= 0) {
    float t[4];
    box_target(a.anchors + 4 * (size_t)j, a.gt_boxes + ((size_t)b * a.G + s) * 4, a, t);
#pragma unroll
    for (int q = 0; q < 4; ++q) dr[q] = smooth_l1_grad(ldval(L.reg, L.rb + q, a.dtype) - t[q], a.beta) / avg;
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) dr[q] = 0.f;
  }
  if (L.an == 0) {                              // the row's pad channels
    for (int k = L.A * (a.nc + 1); k < L.cls_stride; ++k) L.dcls[L.row * L.cls_stride + k] = 0.f;
    for (int k = L.A * 4; k < L.reg_stride; ++k) L.dreg[L.row * L.reg_stride + k] = 0.f;
  }
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

}  // namespace

// include/t3d.h
extern "C" int t3d_ssd_multibox_work_bytes(int B, int A) {
  if (B < 0 || A < 0 || B > (1 << 26)) return T3D_ERR_ARG;
  return 16 * (B > 1 ? B : 1);
}

extern "C" int t3d_ssd_multibox_loss(int dtype, int nlevels, const void* const* cls, const void* const* reg, const int* hw,
                                     const int* nanchors, const int* cls_stride, const int* reg_stride, const float* anchors,
                                     const float* gt_boxes, const int* gt_labels, const int* gt_counts, int B, int G,
                                     int num_classes, float pos_iou_thr, float neg_iou_thr, float min_pos_iou,
                                     int neg_pos_ratio, float beta, const float* stds, void* work, long long work_bytes,
                                     double* scalars, int* num_pos, int* assigned, void* const* dcls, void* const* dreg,
                                     void* stream) {
  if (B < 0 || G < 0 || nlevels < 1 || nlevels > 2 || num_classes <= 0 || neg_pos_ratio < 0 || !(beta > 0.f)) return T3D_ERR_ARG;
  if (dtype != T3D_F32 && dtype != T3D_BF16) return T3D_ERR_ARG;
  if (!(pos_iou_thr == pos_iou_thr) || !(neg_iou_thr == neg_iou_thr) || !(min_pos_iou == min_pos_iou)) return T3D_ERR_ARG;
  if (B == 0) return T3D_OK;
  if (!cls || !reg || !hw || !nanchors || !cls_stride || !reg_stride || !anchors || !gt_counts || !stds || !work || !scalars ||
      !num_pos || !assigned)
    return T3D_ERR_ARG;
  if (G > 0 && (!gt_boxes || !gt_labels)) return T3D_ERR_ARG;
  if ((dcls == nullptr) != (dreg == nullptr)) return T3D_ERR_ARG;
  if (misaligned(anchors, 4) || misaligned(gt_boxes, 4) || misaligned(gt_labels, 4) || misaligned(gt_counts, 4) ||
      misaligned(num_pos, 4) || misaligned(assigned, 4) || misaligned(work, 8) || misaligned(scalars, 8))
    return T3D_ERR_ARG;
  MbArgs a{};
  a.nlevels = nlevels; a.dtype = dtype;
  const uintptr_t esz = dtype == T3D_F32 ? 4 : 2;
  long long tot = 0;
  for (int l = 0; l < nlevels; ++l) {
    if (!cls[l] || !reg[l] || hw[l] <= 0 || nanchors[l] <= 0 || cls_stride[l] < (long long)nanchors[l] * (num_classes + 1) ||
        reg_stride[l] < (long long)nanchors[l] * 4 || misaligned(cls[l], esz) || misaligned(reg[l], esz))
      return T3D_ERR_ARG;
    if (dcls && (!dcls[l] || !dreg[l] || misaligned(dcls[l], 4) || misaligned(dreg[l], 4))) return T3D_ERR_ARG;
    a.lv[l] = MbLevel{cls[l], reg[l], dcls ? static_cast<float*>(dcls[l]) : nullptr, dcls ? static_cast<float*>(dreg[l]) : nullptr,
                      hw[l], nanchors[l], cls_stride[l], reg_stride[l]};
    tot += (long long)hw[l] * nanchors[l];
  }
  if (neg_iou_thr != pos_iou_thr) return T3D_ERR_UNSUPPORTED;      // (an ignore band between the two thresholds is not built)
  if (tot > kMaxA || G > kMaxG) return T3D_ERR_UNSUPPORTED;
  if ((long long)B * tot >= (1ll << 31)) return T3D_ERR_UNSUPPORTED;
  const int need = t3d_ssd_multibox_work_bytes(B, (int)tot);
  if (need < 0 || work_bytes < need) return T3D_ERR_ARG;
  a.anchors = anchors; a.gt_boxes = gt_boxes; a.gt_labels = gt_labels; a.gt_counts = gt_counts;
  a.B = B; a.G = G; a.Atot = (int)tot; a.nc = num_classes; a.ratio = neg_pos_ratio; a.grads = dcls ? 1 : 0;
  a.pos_thr = pos_iou_thr; a.min_pos = min_pos_iou; a.beta = beta;
  a.sx = stds[0]; a.sy = stds[1]; a.sw = stds[2]; a.sh = stds[3];
  a.partial = static_cast<double*>(work); a.scalars = scalars; a.num_pos = num_pos; a.assigned = assigned;
  const size_t lds = (size_t)kFixedLds + 8 * (size_t)tot;
  if (lds > 64 * 1024 && t3d_max_lds((const void*)mb_image_kernel, (int)lds) != hipSuccess) return T3D_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  T3D_LAUNCH(mb_image_kernel, dim3(B), dim3(kNT), lds, st, a);
  T3D_CHECK_LAUNCH();
  const int blocks = dcls ? (int)(((long long)B * tot + 255) / 256) : 1;
  T3D_LAUNCH(mb_grad_kernel, dim3(blocks), dim3(256), 0, st, a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
