// The joints of the live pipeline (scripts/demo.py:56-78 of the reference: detector -> regressor -> tracker -> keypoints in
// frame pixels) as device kernels, so that a frame never leaves the GPU between the stages (include/t3d.h:
// t3d_ssd_select_rects, t3d_head_select, t3d_track_kp_to_frame).
//
// All three are latency-bound: a frame's work is a few hundred to a few thousand items.  One workgroup per frame / camera /
// crop, the working set in LDS, plain vector loads and stores.  The arithmetic restates the host code it replaces literally
// (the numpy / Python expressions are quoted next to each step); the library is built with -ffp-contract=off and the pragma
// below pins that for this file: every product and sum is rounded on its own, as the host rounds them.
#include <limits.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSelThreads = 256;
constexpr int kSelMaxCand = 4096;        // candidates per frame (power of two): 12 bytes of LDS each

struct SelArgs {
  const float* out;      // [F][nc][K][6]
  const int* cnt;        // [F][nc]
  int nc, K, max_per_img, P, D, H, W;
  float input_size, conf;
  double r0, r1;
  int* rects;
  int* crop_rects;
  float* scores;
  int* det_labels;
  int* counts;
  int* overflow;
};

// fp32 -> a 32-bit word whose unsigned order is the float order (-0 and +0 alike, as `==` has them)
__device__ __forceinline__ unsigned f32_order(float s) {
  if (s == 0.f) s = 0.f;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ascending bitonic sort of key[0..n2) (n2 a power of two <= blockDim.x * 2 * k), all threads of the workgroup
__device__ void bitonic_sort(unsigned long long* key, int n2) {
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (n2 >> 1); t += kSelThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));      // the lower index of pair t at distance j
        const int p = i | j;
        const bool up = (i & k) == 0;
        const unsigned long long a = key[i], b = key[p];
        if ((a > b) == up) { key[i] = b; key[p] = a; }
      }
      __syncthreads();
    }
  }
}

__device__ __forceinline__ int next_pow2(int n) {
  int p = 1;
  while (p < n) p <<= 1;
  return p;
}

struct SelRow { int left, top, right, bottom, label; float score; bool pass; };

// SSD300.detect's `rows[:, :4] /= INPUT_SIZE` (fp32) followed by one iteration of Detector._decode_detections
// (utils/ie_wrappers.py:166-183) on row r = (x1, y1, x2, y2, score, label)
__device__ SelRow decode_row(const float* r, const SelArgs& a) {
  SelRow o;
  const float x1 = r[0] / a.input_size, y1 = r[1] / a.input_size, x2 = r[2] / a.input_size, y2 = r[3] / a.input_size;
  o.score = r[4];
  o.label = (int)r[5];
  o.pass = o.score > a.conf;                                       // `confidence > self.confidence`, both fp32
  const float fw = (float)a.W, fh = (float)a.H;
  o.left = (int)((x1 > 0.f ? x1 : 0.f) * fw);                      // int(max(x1, 0) * frame_shape[1]): fp32 product, truncated
  o.top = (int)((y1 > 0.f ? y1 : 0.f) * fh);
  o.right = (int)((x2 > 0.f ? x2 : 0.f) * fw);
  o.bottom = (int)((y2 > 0.f ? y2 : 0.f) * fh);
  if (a.r0 != 1.0 || a.r1 != 1.0) {                                // `self.expand_ratio != (1., 1.)`
    const int w = o.right - o.left, h = o.bottom - o.top;
    const double dw = (double)w * (a.r0 - 1.0) / 2.0, dh = (double)h * (a.r1 - 1.0) / 2.0;
    const int l = (int)((double)o.left - dw), t = (int)((double)o.top - dh);
    o.right = (int)((double)o.right + dw);
    o.bottom = (int)((double)o.bottom + dh);
    o.left = l > 0 ? l : 0;
    o.top = t > 0 ? t : 0;
  }
  return o;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kSelThreads) void ssd_select_rects_kernel(const SelArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned long long* key = reinterpret_cast<unsigned long long*>(smem);       // [P]
  int* src = reinterpret_cast<int*>(smem + (size_t)a.P * 8);                   // [P]: sorted rank -> row (c * K + k)
  __shared__ int cstart[65];
  __shared__ int nsurv;
  const int f = blockIdx.x, tid = threadIdx.x;
  const float* out = a.out + (size_t)f * a.nc * a.K * 6;

  // ---- 1. the rows class-major, the first counts[f][c] of each class (SSD300's merge) -------------------------------
  if (tid == 0) {
    int n = 0;
    for (int c = 0; c < a.nc; ++c) {
      cstart[c] = n;
      n += clampi(a.cnt[f * a.nc + c], 0, a.K);
    }
    cstart[a.nc] = n;
    nsurv = 0;
  }
  __syncthreads();
  const int N = cstart[a.nc];                                       // <= nc * K <= P
  const int n2 = next_pow2(N > 1 ? N : 1);
  for (int i = tid; i < n2; i += kSelThreads) key[i] = ~0ull;
  __syncthreads();
  for (int e = tid; e < a.nc * a.K; e += kSelThreads) {
    const int c = e / a.K, k = e - c * a.K;
    const int n = cstart[c + 1] - cstart[c];
    if (k >= n) continue;
    const int i = cstart[c] + k;                                    // position in the concatenation
    // ---- 2. np.argsort(-score, kind='stable'): descending score, then ascending position
    key[i] = ((unsigned long long)(~f32_order(out[(size_t)e * 6 + 4])) << 32) | (unsigned)i;
    src[i] = e;                                                     // (position -> row, until the ranks replace it below)
  }
  __syncthreads();
  bitonic_sort(key, n2);
  const int M = N < a.max_per_img ? N : a.max_per_img;              // `[:max_per_img]`
  // rank -> row: read every position's row before any rank is written (positions and ranks share the array)
  int rowof[kSelMaxCand / kSelThreads];
#pragma unroll
  for (int q = 0; q < kSelMaxCand / kSelThreads; ++q) {
    const int r = tid + q * kSelThreads;
    rowof[q] = r < M ? src[(unsigned)(key[r] & 0xffffffffu)] : -1;
  }
  __syncthreads();
  const int m2 = next_pow2(M > 1 ? M : 1);
  int mine = 0;
#pragma unroll
  for (int q = 0; q < kSelMaxCand / kSelThreads; ++q) {
    const int r = tid + q * kSelThreads;
    if (r >= m2) continue;
    unsigned long long k2 = ~0ull;
    if (r < M) {
      src[r] = rowof[q];
      // ---- 3.-6. scale, threshold, pixels, expand
      const SelRow row = decode_row(out + (size_t)rowof[q] * 6, a);
      if (row.pass) {
        // ---- 7. list.sort(key=top, reverse=True): descending top, equal tops in their order
        k2 = ((unsigned long long)(~((unsigned)row.top ^ 0x80000000u)) << 32) | (unsigned)r;
        ++mine;
      }
    }
    key[r] = k2;
  }
  if (mine) atomicAdd(&nsurv, mine);
  __syncthreads();
  bitonic_sort(key, m2);
  const int ns = nsurv;
  const int nout = ns < a.D ? ns : a.D;                              // ---- 8. `[:D]`
  int* rects = a.rects + (size_t)f * a.D * 4;
  int* crops = a.crop_rects + (size_t)f * a.D * 4;
  for (int j = tid; j < a.D; j += kSelThreads) {
    int l = 0, t = 0, r = 0, b = 0, cl = 0, ct = 0, cr = 0, cb = 0, lab = 0;
    float sc = 0.f;
    if (j < nout) {
      const SelRow row = decode_row(out + (size_t)src[(unsigned)(key[j] & 0xffffffffu)] * 6, a);
      l = row.left; t = row.top; r = row.right; b = row.bottom; lab = row.label; sc = row.score;
      // frame[top:bottom, left:right] of frame f in the stack of F frames: bounds clamped to the frame, rows shifted
      cl = clampi(l, 0, a.W); cr = clampi(r, 0, a.W);
      ct = clampi(t, 0, a.H) + f * a.H; cb = clampi(b, 0, a.H) + f * a.H;
    }
    rects[4 * j] = l; rects[4 * j + 1] = t; rects[4 * j + 2] = r; rects[4 * j + 3] = b;
    crops[4 * j] = cl; crops[4 * j + 1] = ct; crops[4 * j + 2] = cr; crops[4 * j + 3] = cb;
    a.scores[(size_t)f * a.D + j] = sc;
    a.det_labels[(size_t)f * a.D + j] = lab;
  }
  if (tid == 0) {
    a.counts[f] = nout;
    a.overflow[f] = ns - nout;
  }
}

// one workgroup of one wave per crop: lane k < 18 copies keypoint coordinate k of the chosen head
__global__ __launch_bounds__(64) void head_select_kernel(const float* __restrict__ kp_all, const float* __restrict__ logits,
                                                         int n, int C, int* __restrict__ labels, float* __restrict__ kp) {
  const int i = blockIdx.x, lane = threadIdx.x;
  int best = 0;
  if (logits && C > 1) {
    float bv = logits[(size_t)i * C];
    for (int c = 1; c < C; ++c) {                                   // the lowest index among the maxima
      const float v = logits[(size_t)i * C + c];
      if (v > bv) { bv = v; best = c; }
    }
  }
  if (lane == 0) labels[i] = best;
  if (lane < 18) kp[(size_t)i * 18 + lane] = kp_all[((size_t)best * n + i) * 18 + lane];
}

// Regressor.transform_kp (utils/ie_wrappers.py:144-152) per tracked object: kp[:, 0] * (x1 - x0), then += x0, in fp64
__global__ __launch_bounds__(64) void track_kp_to_frame_kernel(const int* __restrict__ out_count, const int* __restrict__ out_boxes,
                                                               const double* __restrict__ out_kp, double* __restrict__ kp_frame,
                                                               int T) {
  const int s = blockIdx.x;
  const int n = clampi(out_count[s], 0, T);
  const int* boxes = out_boxes + (size_t)s * T * 4;
  const double* kp = out_kp + (size_t)s * T * 18;
  double* o = kp_frame + (size_t)s * T * 18;
  for (int e = threadIdx.x; e < n * 18; e += 64) {
    const int t = e / 18, k = e - t * 18, ax = k & 1;               // even entries are x, odd are y
    const int lo = boxes[4 * t + ax], hi = boxes[4 * t + 2 + ax];
    const double scaled = kp[e] * (double)(hi - lo);
    o[e] = scaled + (double)lo;
  }
}

}  // namespace

// include/t3d.h
extern "C" int t3d_ssd_select_rects(const float* out, const int* cnt, int F, int num_classes, int max_per_class, int max_per_img,
                                    float input_size, float conf, int frame_h, int frame_w, double expand_w, double expand_h,
                                    int max_dets, int* rects, int* crop_rects, float* scores, int* det_labels, int* counts,
                                    int* overflow, void* stream) {
  if (!out || !cnt || !rects || !crop_rects || !scores || !det_labels || !counts || !overflow) return T3D_ERR_ARG;
  if (F < 1 || num_classes < 1 || num_classes > 64 || max_per_class < 1 || max_per_img < 1 || max_dets < 1) return T3D_ERR_ARG;
  if (frame_h < 1 || frame_w < 1 || !(input_size > 0.f)) return T3D_ERR_ARG;
  if ((long long)F * frame_h > INT_MAX) return T3D_ERR_ARG;         // the shifted rows of crop_rects
  const long long cand = (long long)num_classes * max_per_class;
  if (cand > kSelMaxCand) return T3D_ERR_UNSUPPORTED;
  int P = 1;
  while (P < cand) P <<= 1;
  SelArgs a{};
  a.out = out; a.cnt = cnt;
  a.nc = num_classes; a.K = max_per_class; a.max_per_img = max_per_img; a.P = P; a.D = max_dets; a.H = frame_h; a.W = frame_w;
  a.input_size = input_size; a.conf = conf; a.r0 = expand_w; a.r1 = expand_h;
  a.rects = rects; a.crop_rects = crop_rects; a.scores = scores; a.det_labels = det_labels; a.counts = counts; a.overflow = overflow;
  T3D_LAUNCH(ssd_select_rects_kernel, dim3(F), dim3(kSelThreads), (size_t)P * 12, reinterpret_cast<hipStream_t>(stream), a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_head_select(const float* kp_all, const float* logits, int n, int num_heads, int num_classes, int* labels,
                               float* kp, void* stream) {
  if (!kp_all || !labels || !kp || n < 0 || num_heads < 1 || num_classes < 0) return T3D_ERR_ARG;
  if (logits && num_classes > num_heads) return T3D_ERR_ARG;        // a class without a head
  if (n == 0) return T3D_OK;
  T3D_LAUNCH(head_select_kernel, dim3(n), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), kp_all, logits, n, num_classes,
             labels, kp);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

extern "C" int t3d_track_kp_to_frame(const int* out_count, const int* out_boxes, const double* out_kp, double* kp_frame, int S,
                                     int max_tracks, void* stream) {
  if (!out_count || !out_boxes || !out_kp || !kp_frame || S < 1 || max_tracks < 1) return T3D_ERR_ARG;
  T3D_LAUNCH(track_kp_to_frame_kernel, dim3(S), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), out_count, out_boxes, out_kp,
             kp_frame, max_tracks);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
