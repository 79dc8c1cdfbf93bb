// Squeeze-excite gate of MobileNetV3 (SELayer, torchdet3d/models/mobilenetv3.py:92-107), fp32:
//   m = mean_hw BN(y)  ->  h = relu(W1 m + b1)  ->  q = W2 h + b2  ->  s = h_sigmoid(q),   x * s
// The spatial mean never touches the feature map again: the depthwise kernel already emitted
// sum_hw(y) per (sample, channel), and BN is affine, so m = scale * sum/HW + shift.
// Backward (same shape of work, reversed) consumes the per-sample sums  P1 = sum_hw dv,
// P2 = sum_hw dv*y  that the projection conv's data-gradient kernel emitted (dv = gradient at the
// gated tensor), and produces
//   g[b][c]     = dL/dm / HW                      (the pooled path's contribution to every pixel)
//   bn sums     sum(du), sum(du*y) of the depthwise conv's BatchNorm  (du = s*dv + g)
//   dq, dp      pre-activation gradients of the two FCs, for the weight-gradient kernels.
// Entry points and their launches:
//   t3d_se_fwd_fused    se_slice_kernel<0> (m, h), <1> (q, s)
//   t3d_se_bwd_data     se_slice_kernel<2> (dq, dp), <3> (g, bn sums)
//   t3d_se_bwd_weights  se_wgrad_tile_kernel x 2 (dW2, dW1), se_bias_kernel -- leaves of the backward, issued by the host on
//                       its weight-gradient stream
//   t3d_se_after_bwd    se_after_bwd_kernel: the gate AFTER the activation, its whole backward as one launch (end of file)
#include "common.h"

namespace {

struct SeArgs {
  const float *gap, *scale, *shift;
  const float *w1, *b1, *w2, *b2;
  float *m, *h, *q, *s;
  const float* ps;   // [B][C][2]
  float *g, *dq, *dp;
  double* stats;     // [2][C]
  float *dw1, *db1, *dw2, *db2;
  int B, C, R, HW;
  int gapq;          // `gap` holds int64 fixed point (t3d_set_exact_pool; common.h: t3d_pool_get)
};

// ------------------------------------------------------------------ FC weight / bias gradients (t3d_se_bwd_weights)
// out[b][o] = sum_i in(b, i) * W(o, i) for a 64-row x OT-output tile; thread = (row bl, OT/4 outputs og*PT..); each operand
// element is read once per tile.  WT: W is stored [I][O], else [O][I].  [ibeg, iend) restricts the contraction (the callers
// here take all of it).
// OT = 4: the products are tiny, so what matters is enough workgroups to hide the load latency.
constexpr int OT = 4, PT = OT / 4;
// IT: the input is read transposed (rows of the tile are its fast axis in memory) -- the weight-gradient products.
template <bool WT, bool IT = false, typename InF>
__device__ __forceinline__ void fc_tile(InF in, const float* __restrict__ W, int I, int O, int b0, int o0, int B,
                                        float acc[PT], float (*lin)[65], float (*lw)[65], int ibeg = 0, int iend = 1 << 30) {
  const int t = threadIdx.x, bl = t & 63, og = t >> 6;
#pragma unroll
  for (int j = 0; j < PT; ++j) acc[j] = 0.f;
  iend = min(iend, I);
  for (int i0 = ibeg; i0 < iend; i0 += 64) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const int idx = t + 256 * k, row = IT ? (idx & 63) : (idx >> 6), col = IT ? (idx >> 6) : (idx & 63);
      const int b = b0 + row, i = i0 + col;
      lin[row][col] = (b < B && i < iend) ? in(b, i) : 0.f;
    }
#pragma unroll
    for (int k = 0; k < OT / 4; ++k) {
      const int idx = t + 256 * k;
      int row, col;
      if (WT) { row = idx % OT; col = idx / OT; } else { row = idx >> 6; col = idx & 63; }
      const int o = o0 + row, i = i0 + col;
      float v = 0.f;
      if (o < O && i < iend) v = WT ? W[(size_t)i * O + o] : W[(size_t)o * I + i];
      lw[row][col] = v;
    }
    __syncthreads();
#pragma unroll 8
    for (int ii = 0; ii < 64; ++ii) {
      const float x = lin[bl][ii];
#pragma unroll
      for (int j = 0; j < PT; ++j) acc[j] = fmaf(x, lw[og * PT + j][ii], acc[j]);
    }
  }
}

// weight gradients as tiled products (fc_tile), contraction over the batch:
//   dW2[c][r] = sum_b dq[b][c] h[b][r]   (rows c, outputs r)      dW1[r][c] = sum_b dp[b][r] m[b][c]   (rows r, outputs c)
// which = 0: dW2, grid (ceil(R/OT), ceil(C/64));  which = 1: dW1, grid (ceil(C/OT), ceil(R/64))
__global__ __launch_bounds__(256) void se_wgrad_tile_kernel(const SeArgs a, int which) {
  __shared__ float lin[64][65], lw[OT][65];
  const int o0 = blockIdx.x * OT, r0 = blockIdx.y * 64;
  const int rows = which == 0 ? a.C : a.R, outs = which == 0 ? a.R : a.C;
  const float* src = which == 0 ? a.dq : a.dp;        // [B][rows]
  const float* wsrc = which == 0 ? a.h : a.m;         // [B][outs] = [I][O]
  auto in = [&](int row, int b) { return src[(size_t)b * rows + row]; };
  float acc[PT];
  fc_tile<true, true>(in, wsrc, a.B, outs, r0, o0, rows, acc, lin, lw);
  const int row = r0 + (threadIdx.x & 63), og = threadIdx.x >> 6;
  float* dst = which == 0 ? a.dw2 : a.dw1;
  if (row < rows) {
#pragma unroll
    for (int j = 0; j < PT; ++j) {
      const int o = o0 + og * PT + j;
      if (o < outs) dst[(size_t)row * outs + o] = acc[j];
    }
  }
}

// bias gradients: db2[c] = sum_b dq[b][c], db1[r] = sum_b dp[b][r]; block = 64 channels x 4 batch slices
__global__ __launch_bounds__(256) void se_bias_kernel(const SeArgs a) {
  __shared__ float red[4][64];
  const int ch = blockIdx.x * 64 + (threadIdx.x & 63), sl = threadIdx.x >> 6;
  const bool second = ch >= a.C;                       // channels [0, C): db2, [C, C+R): db1
  const int c = second ? ch - a.C : ch, n = second ? a.R : a.C;
  const float* src = second ? a.dp : a.dq;
  float acc = 0.f;
  if (c < n)
    for (int b = sl; b < a.B; b += 4) acc += src[(size_t)b * n + c];
  red[sl][threadIdx.x & 63] = acc;
  __syncthreads();
  if (sl == 0 && c < n) {
    const float v = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
    (second ? a.db1 : a.db2)[c] = v;
  }
}

// ------------------------------------------------------------------ the gate's products: one launch per PRODUCT, outputs sliced over workgroups
// A workgroup owns SPG samples x SL_OB outputs of ONE product and its eight waves split the contraction: thread = output, weights
// read coalesced along the output axis (every matrix comes as [I][O]), the staged inputs broadcast from LDS, the waves' partial
// sums added in wave order.  960 -> 240 leaves a wave 120 inputs to walk, 240 -> 960 thirty, and 256 ... 960 small workgroups
// fill the chip.
// What the shape answers to (rocprofv3, MobileNetV3-large, 8 gates): walking BOTH products of a direction inside one workgroup
// per four samples was ~60 dependent rounds of L2 loads per thread -- 27 / 37 us alone, but 33 / 105 us inside the step, where
// the rounds get longer while the weight-gradient stream is busy in L2 -- and 1024-thread blocks of 8 samples ran 37 us alone
// but 114 us inside the step: a block that needs a whole CU's wave slots waits for the weight-gradient stream's blocks to drain.
// The price of the slices is a second launch per direction (a dependent kernel boundary, ~3 us).  Summation order: eight
// contiguous slices of the contraction, added in slice order -- deterministic.
constexpr int SPG = 4;          // samples per workgroup
constexpr int SL_OB = 64, SL_T = 512, SL_G = SL_T / SL_OB;      // eight waves split the contraction (256 threads: 67 us in the backward)
// MODE 0: h = relu(W1 m + b1), m from the pooled sums   1: q = W2 h + b2, s = h_sigmoid(q)
//      2: dp = relu'(h) (dq W2), dq from the per-sample sums   3: g = (dp W1) / HW + the BatchNorm-backward sums
template <int MODE>
__global__ __launch_bounds__(SL_T) void se_slice_kernel(const SeArgs a, const float* __restrict__ Wt, const int nrep, const long long rstride) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr bool FROM_C = MODE == 0 || MODE == 2;      // contraction over the C channels (else over the R hidden units)
  const int I = FROM_C ? a.C : a.R, O = FROM_C ? a.R : a.C;
  float* in = lds;                                     // [I][SPG]
  float* red = in + (size_t)I * SPG;                   // [SL_T][SPG]
  const int b0 = blockIdx.x * SPG, t = threadIdx.x;
  const bool first = blockIdx.y == 0;                  // the slice that also stores the staged input (m / dq)
  const float inv = 1.f / (float)a.HW;
  for (int i = t; i < I * SPG; i += SL_T) {
    const int c = i / SPG, s = i % SPG, b = b0 + s;
    float v = 0.f;
    if (b < a.B) {
      const size_t k = (size_t)b * I + c;
      if (MODE == 0) {
        v = a.scale[c] * (t3d_pool_get(a.gap, k, a.gapq) * inv) + a.shift[c];
        if (first) a.m[k] = v;
      } else if (MODE == 1) {
        v = a.h[k];
      } else if (MODE == 2) {
        const float ds = a.scale[c] * a.ps[2 * k + 1] + a.shift[c] * a.ps[2 * k];
        const float q = a.q[k];
        v = (q > -3.f && q < 3.f) ? ds * (1.f / 6.f) : 0.f;     // relu6 passes strictly inside
        if (first) a.dq[k] = v;
      } else {
        v = a.dp[k];
      }
    }
    in[i] = v;
  }
  __syncthreads();
  const int grp = t / SL_OB, ol = t % SL_OB, o = blockIdx.y * SL_OB + ol;
  const bool live = o < O;
  const int per = (I + SL_G - 1) / SL_G, i0 = min(grp * per, I), i1 = min(i0 + per, I);
  float acc[SPG];
#pragma unroll
  for (int s = 0; s < SPG; ++s) acc[s] = 0.f;
  if (live) {
    // 32 weight loads in flight per thread (the walk is a chain of L2 round trips, ~4x longer beside the weight-gradient stream
    // than alone); the 64 sample groups that read one output slice start at DIFFERENT rows of their slice of the contraction, so
    // that they do not all ask L2 for the same line at the same time.  The order of a thread's adds is fixed by (workgroup,
    // thread) alone: deterministic, as before.
    const int n = i1 - i0, rot = n > 0 ? (int)((blockIdx.x * 37u) % (unsigned)n) : 0;
    int done = 0;
    for (; done + 32 <= n; done += 32) {
      float w[32];
      int ii[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        int r = rot + done + u;
        if (r >= n) r -= n;
        ii[u] = i0 + r;
        w[u] = Wt[(size_t)ii[u] * O + o];
      }
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        const float4 x0 = *reinterpret_cast<const float4*>(in + ii[u] * SPG);
        acc[0] = fmaf(x0.x, w[u], acc[0]); acc[1] = fmaf(x0.y, w[u], acc[1]);
        acc[2] = fmaf(x0.z, w[u], acc[2]); acc[3] = fmaf(x0.w, w[u], acc[3]);
      }
    }
    for (; done + 8 <= n; done += 8) {         // (the hidden-unit contractions: 24 ... 240 inputs over eight waves)
      float w[8];
      int ii[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        int r = rot + done + u;
        if (r >= n) r -= n;
        ii[u] = i0 + r;
        w[u] = Wt[(size_t)ii[u] * O + o];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const float4 x0 = *reinterpret_cast<const float4*>(in + ii[u] * SPG);
        acc[0] = fmaf(x0.x, w[u], acc[0]); acc[1] = fmaf(x0.y, w[u], acc[1]);
        acc[2] = fmaf(x0.z, w[u], acc[2]); acc[3] = fmaf(x0.w, w[u], acc[3]);
      }
    }
    for (; done < n; ++done) {
      int r = rot + done;
      if (r >= n) r -= n;
      const float w = Wt[(size_t)(i0 + r) * O + o];
#pragma unroll
      for (int s = 0; s < SPG; ++s) acc[s] = fmaf(in[(i0 + r) * SPG + s], w, acc[s]);
    }
  }
  if (grp > 0) {
#pragma unroll
    for (int s = 0; s < SPG; ++s) red[(size_t)t * SPG + s] = acc[s];
  }
  __syncthreads();
  if (grp != 0 || !live) return;
#pragma unroll
  for (int g = 1; g < SL_G; ++g)
#pragma unroll
    for (int s = 0; s < SPG; ++s) acc[s] += red[(size_t)(g * SL_OB + ol) * SPG + s];
  if (MODE == 0) {
    const float b1 = a.b1[o];
#pragma unroll
    for (int s = 0; s < SPG; ++s)
      if (b0 + s < a.B) a.h[(size_t)(b0 + s) * a.R + o] = fmaxf(acc[s] + b1, 0.f);
  } else if (MODE == 1) {
    const float b2 = a.b2[o];
#pragma unroll
    for (int s = 0; s < SPG; ++s) {
      if (b0 + s < a.B) {
        const float q = acc[s] + b2;
        a.q[(size_t)(b0 + s) * a.C + o] = q;
        a.s[(size_t)(b0 + s) * a.C + o] = hsigmoid(q);
      }
    }
  } else if (MODE == 2) {
#pragma unroll
    for (int s = 0; s < SPG; ++s)
      if (b0 + s < a.B) a.dp[(size_t)(b0 + s) * a.R + o] = a.h[(size_t)(b0 + s) * a.R + o] > 0.f ? acc[s] : 0.f;
  } else {
    float v1 = 0.f, v2 = 0.f;
#pragma unroll
    for (int s = 0; s < SPG; ++s) {
      if (b0 + s < a.B) {
        const size_t k = (size_t)(b0 + s) * a.C + o;
        const float gu = acc[s] * inv;                          // every pixel of u receives dL/dm / HW
        a.g[k] = gu;
        const float sg = a.s[k], p1 = a.ps[2 * k], p2 = a.ps[2 * k + 1];
        v1 += sg * p1 + (float)a.HW * gu;
        v2 += sg * p2 + gu * t3d_pool_get(a.gap, k, a.gapq);
      }
    }
    if (a.stats) {      // one add per (sample group, channel), spread over the reduction replicas
      double* st = a.stats + (size_t)(blockIdx.x % nrep) * rstride;
      atomicAdd(st + o, (double)v1);
      atomicAdd(st + a.C + o, (double)v2);
    }
  }
}

// (Measured and removed: the same products on v_mfma_f32_16x16x4_f32 -- a workgroup per 16 samples x 64 outputs, the 16 input
// rows staged in LDS, exact fp32 products: correct (the suite passed on it) and 0.3 ms SLOWER per MobileNetV3-large step than the
// slices (7.93 against 7.63 ms, two same-box pairs): staging 16 x 960 transformed inputs per workgroup is a 60-round chain of global
// loads where the slice kernel's 4 x 960 over 512 threads is eight, and 64 workgroups do not fill the chip.)
template <int MODE>
static void se_slice_launch(const SeArgs& a, const float* Wt, hipStream_t st) {
  const int I = (MODE == 0 || MODE == 2) ? a.C : a.R, O = (MODE == 0 || MODE == 2) ? a.R : a.C;
  const size_t lds = ((size_t)I * SPG + (size_t)SL_T * SPG) * sizeof(float);
  T3D_LAUNCH(se_slice_kernel<MODE>, dim3(cdiv(a.B, SPG), cdiv(O, SL_OB)), dim3(SL_T), lds, st, a, Wt, g_t3d_reduce.nrep < 1 ? 1 : g_t3d_reduce.nrep,
             g_t3d_reduce.nrep < 1 ? 0 : g_t3d_reduce.stats_stride);
}

}  // namespace

// forward of the gate: m, h, q, s.  w1t [C][R], w2t [R][C]: transposed fp32 copies of fc.0 / fc.2 (the caller keeps them
// current, e.g. t3d_pack_weights_batched), so that the forward's contractions read [I][O] too.  C, R <= 1024.
extern "C" int t3d_se_fwd_fused(const float* gap_sum, const float* scale, const float* shift, const float* w1t,
                                const float* b1, const float* w2t, const float* b2, float* m, float* h, float* q, float* s,
                                int B, int C, int R, int HW, void* stream) {
  if (!gap_sum || !scale || !shift || !w1t || !b1 || !w2t || !b2 || !m || !h || !q || !s || B <= 0 || C <= 0 || R <= 0 ||
      HW <= 0)
    return T3D_ERR_ARG;
  SeArgs a{};
  a.gap = gap_sum; a.gapq = g_t3d_reduce.pool_exact; a.scale = scale; a.shift = shift; a.b1 = b1; a.b2 = b2;
  a.m = m; a.h = h; a.q = q; a.s = s; a.B = B; a.C = C; a.R = R; a.HW = HW;
  se_slice_launch<0>(a, w1t, reinterpret_cast<hipStream_t>(stream));
  se_slice_launch<1>(a, w2t, reinterpret_cast<hipStream_t>(stream));
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

// data part of the backward: dq, dp (kept for t3d_se_bwd_weights), g and the BatchNorm-backward sums.  W1 [R][C] and
// W2 [C][R] are the parameters themselves: the backward contracts over their ROW index, so they already are [I][O].

extern "C" int t3d_se_bwd_data(const float* ps_stats, const float* gap_sum, const float* scale, const float* shift,
                               const float* w1, const float* w2, const float* h, const float* q, const float* s, float* g,
                               float* dq, float* dp, double* stats, int B, int C, int R, int HW, void* stream) {
  if (!ps_stats || !gap_sum || !scale || !shift || !w1 || !w2 || !h || !q || !s || !g || !dq || !dp || B <= 0 || C <= 0 ||
      R <= 0 || HW <= 0)
    return T3D_ERR_ARG;
  SeArgs a{};
  a.ps = ps_stats; a.gap = gap_sum; a.gapq = g_t3d_reduce.pool_exact; a.scale = scale; a.shift = shift; a.w1 = w1; a.w2 = w2;
  a.h = const_cast<float*>(h); a.q = const_cast<float*>(q); a.s = const_cast<float*>(s);
  a.g = g; a.dq = dq; a.dp = dp; a.stats = stats; a.B = B; a.C = C; a.R = R; a.HW = HW;
  se_slice_launch<2>(a, w2, reinterpret_cast<hipStream_t>(stream));
  se_slice_launch<3>(a, w1, reinterpret_cast<hipStream_t>(stream));
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

// weight / bias gradients of the two FCs from the dq, dp that t3d_se_bwd_data left (leaves of the backward graph: the
// host side issues them on its weight-gradient stream)
extern "C" int t3d_se_bwd_weights(const float* m, const float* h, const float* dq, const float* dp, float* dw1, float* db1,
                                  float* dw2, float* db2, int B, int C, int R, void* stream) {
  if (!m || !h || !dq || !dp || !dw1 || !db1 || !dw2 || !db2 || B <= 0 || C <= 0 || R <= 0) return T3D_ERR_ARG;
  SeArgs a{};
  a.m = const_cast<float*>(m); a.h = const_cast<float*>(h); a.dq = const_cast<float*>(dq); a.dp = const_cast<float*>(dp);
  a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2; a.B = B; a.C = C; a.R = R; a.HW = 1;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  T3D_LAUNCH(se_wgrad_tile_kernel, dim3(cdiv(R, OT), cdiv(C, 64)), dim3(256), 0, st, a, 0);
  T3D_LAUNCH(se_wgrad_tile_kernel, dim3(cdiv(C, OT), cdiv(R, 64)), dim3(256), 0, st, a, 1);
  T3D_LAUNCH(se_bias_kernel, dim3(cdiv(C + R, 64)), dim3(256), 0, st, a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

// ------------------------------------------------------------------ gate AFTER the activation: the whole backward as one launch
// v = s * a, a = act(scale*y + shift), s = gate(mean_hw a).  The three-launch sequence (t3d_se_after_sums -> t3d_se_bwd_data ->
// t3d_se_after_apply, elementwise.hip / above) reads dv and y from HBM twice and pays two dependent kernel boundaries.  The
// gate's input gradient g[b,:] needs only sample b's own sums and the two FC matrices (only the FC WEIGHT gradients mix samples,
// and those are issued separately from dq / dp), so here a workgroup owns one sample:
//   pass 1   ds[c] = sum_hw dv*a            thread = (8-channel group, pixel slot); slot partials meet in LDS in slot order
//   gate     dq = h_sigmoid'(q) ds,  dp = relu'(h) (dq W2),  g = (dp W1) / HW       (thread = output: sa_matvec below)
//   pass 2   du = (s*dv + g) * act'(u) over the same plane -- at most 0.53 MB per sample in bf16 (672 x 14^2), so the re-read is
//            served by L2 / Infinity Cache -- and sum(du), sum(du*y): slot partials summed in fp64 in slot order, ONE fp64 atomic
//            per (workgroup, channel) into replica (workgroup % replicas), like the kernels around it.
// Every workgroup streams both FC matrices (<= 1.8 MB fp32) out of L2: what the launch saves is one HBM pass over dv, y and two
// launches, what it costs is that walk per SAMPLE instead of per four samples (se_slice_kernel) -- the engine takes it only at
// the shapes where it measured faster.
namespace {

constexpr int SA_T = 1024;

struct SeAfterArgs {
  const void *dv, *y;
  void* du;
  const float *scale, *shift;
  const float *w1, *w2, *h, *q, *s;
  float *g, *dq, *dp;
  double* stats;
  int act, B, HW, C, R;
  int nrep;
  long long rstride;
};

// out[o] = sum_i in[i] * Wt[i*O + o];  in: LDS [I];  outputs walked in blocks of OP <= SA_T threads, the contraction split over
// the SA_T / OP thread groups that the output width leaves free (partials through `part` [SA_T], added in group order).
template <typename Fin>
__device__ __forceinline__ void sa_matvec(const float* __restrict__ Wt, int I, int O, const float* in, float* part, Fin fin) {
  const int t = threadIdx.x;
  const int OP = min((O + 63) & ~63, SA_T);
  const int ngrp = SA_T / OP, grp = t / OP, ol = t - grp * OP;
  const int per = (I + ngrp - 1) / ngrp;
  const int i0 = min(grp * per, I), i1 = min(i0 + per, I);
  for (int ob = 0; ob < O; ob += OP) {
    const int o = ob + ol;
    const bool live = grp < ngrp && o < O;
    float acc = 0.f;
    if (live) {
      int i = i0;
      for (; i + 16 <= i1; i += 16) {              // sixteen independent weight loads in flight (a chain of L2 round trips)
        float w[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) w[u] = Wt[(size_t)(i + u) * O + o];
#pragma unroll
        for (int u = 0; u < 16; ++u) acc = fmaf(in[i + u], w[u], acc);
      }
      for (; i < i1; ++i) acc = fmaf(in[i], Wt[(size_t)i * O + o], acc);
    }
    if (ngrp > 1) {
      __syncthreads();                               // `part` may still be read from the previous block / product
      if (live && grp > 0) part[t] = acc;
      __syncthreads();
      if (live && grp == 0)
        for (int g = 1; g < ngrp; ++g) acc += part[g * OP + ol];
    }
    if (live && grp == 0) fin(o, acc);
  }
}

template <typename T>
__global__ __launch_bounds__(SA_T) void se_after_bwd_kernel(const SeAfterArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int C = a.C, R = a.R, HW = a.HW, CG = C / 8, t = threadIdx.x, b = blockIdx.x;
  const int nslots = SA_T / CG;                      // >= 8 (C <= 1024)
  float* red = lds;                                  // [nslots][C] slot partials
  float* v0 = red + (size_t)nslots * C;              // [C] dq, later the gate s
  float* v1 = v0 + C;                                // [C] g
  float* vr = v1 + C;                                // [R] dp
  float* part = vr + R;                              // [SA_T]
  const int cgl = t % CG, slot = t / CG, c0 = cgl * 8;
  const bool on = slot < nslots;
  const T* __restrict__ dv = reinterpret_cast<const T*>(a.dv) + (size_t)b * HW * C;
  const T* __restrict__ y = reinterpret_cast<const T*>(a.y) + (size_t)b * HW * C;
  T* __restrict__ du = reinterpret_cast<T*>(a.du) + (size_t)b * HW * C;
  float sc[8], sh[8], acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = a.scale ? a.scale[c0 + j] : 1.f;
    sh[j] = a.scale ? a.shift[c0 + j] : 0.f;
    acc[j] = 0.f;
  }
  // ---- pass 1: ds[c] = sum_hw dv * act(scale*y + shift)
  if (on) {
    for (int hw = slot; hw < HW; hw += nslots) {
      float v[8], d[8];
      const size_t off = (size_t)hw * C + c0;
      Vec8<T>::load(y + off, v);
      Vec8<T>::load(dv + off, d);
      act_affine_vec<8>(v, sc, sh, a.act);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = fmaf(d[j], v[j], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[slot * C + c0 + j] = acc[j];
  }
  __syncthreads();
  for (int c = t; c < C; c += SA_T) {
    float ds = 0.f;
    for (int k = 0; k < nslots; ++k) ds += red[k * C + c];
    const size_t i = (size_t)b * C + c;
    const float qq = a.q[i];
    const float v = (qq > -3.f && qq < 3.f) ? ds * (1.f / 6.f) : 0.f;     // relu6 passes strictly inside
    a.dq[i] = v;
    v0[c] = v;
  }
  __syncthreads();
  // ---- the gate's two products
  sa_matvec(a.w2, C, R, v0, part, [&](int o, float s) {                  // dp = relu'(h) * (dq W2);  W2 is [C][R] = [I][O]
    const float v = a.h[(size_t)b * R + o] > 0.f ? s : 0.f;
    a.dp[(size_t)b * R + o] = v;
    vr[o] = v;
  });
  __syncthreads();
  const float inv = 1.f / (float)HW;
  sa_matvec(a.w1, R, C, vr, part, [&](int o, float s) {                  // g = (dp W1) / HW;  W1 is [R][C] = [I][O]
    const float gu = s * inv;                                            // every pixel of a receives dL/dm / HW
    a.g[(size_t)b * C + o] = gu;
    v1[o] = gu;
  });
  __syncthreads();
  for (int c = t; c < C; c += SA_T) v0[c] = a.s[(size_t)b * C + c];
  __syncthreads();
  // ---- pass 2: du = (s*dv + g) * act'(u), sum(du), sum(du*y)
  float gs[8], gg[8], s1[8], s2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    gs[j] = v0[c0 + j];
    gg[j] = v1[c0 + j];
    s1[j] = s2[j] = 0.f;
  }
  if (on) {
    for (int hw = slot; hw < HW; hw += nslots) {
      float d[8], yv[8];
      const size_t off = (size_t)hw * C + c0;
      Vec8<T>::load(dv + off, d);
      Vec8<T>::load(y + off, yv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float da = fmaf(gs[j], d[j], gg[j]);
        const float v = Vec8<T>::round(da * act_grad(yv[j] * sc[j] + sh[j], a.act));
        d[j] = v;
        s1[j] += v;
        s2[j] = fmaf(v, yv[j], s2[j]);
      }
      Vec8<T>::store(du + off, d);
    }
  }
  if (!a.stats) return;
  double* st = a.stats + (size_t)(b % a.nrep) * a.rstride;
#pragma unroll
  for (int which = 0; which < 2; ++which) {
    __syncthreads();                                 // (`red` of the previous round has been read)
    if (on) {
#pragma unroll
      for (int j = 0; j < 8; ++j) red[slot * C + c0 + j] = which ? s2[j] : s1[j];
    }
    __syncthreads();
    for (int c = t; c < C; c += SA_T) {
      double v = 0.0;
      for (int k = 0; k < nslots; ++k) v += (double)red[k * C + c];
      atomicAdd(st + (size_t)which * C + c, v);
    }
  }
}

}  // namespace

extern "C" int t3d_se_after_bwd(int dtype, const void* dv, const void* y, const t3d_prologue* pro, const float* w1,
                                const float* w2, const float* h, const float* q, const float* s, float* g, float* dq,
                                float* dp, void* du, double* stats, int B, int HW, int C, int R, void* stream) {
  if (!dv || !y || !w1 || !w2 || !h || !q || !s || !g || !dq || !dp || !du || B <= 0 || HW <= 0 || C <= 0 || R <= 0 || (C % 8))
    return T3D_ERR_ARG;
  if (C > 1024 || R > 1024) return T3D_ERR_UNSUPPORTED;
  if (pro && pro->se) return T3D_ERR_UNSUPPORTED;
  SeAfterArgs a{};
  a.dv = dv; a.y = y; a.du = du; a.w1 = w1; a.w2 = w2; a.h = h; a.q = q; a.s = s; a.g = g; a.dq = dq; a.dp = dp;
  a.stats = stats; a.B = B; a.HW = HW; a.C = C; a.R = R; a.act = T3D_ACT_NONE;
  if (pro) { a.scale = pro->scale; a.shift = pro->shift; a.act = pro->act; }
  a.nrep = g_t3d_reduce.nrep < 1 ? 1 : g_t3d_reduce.nrep;
  a.rstride = g_t3d_reduce.nrep < 1 ? 0 : g_t3d_reduce.stats_stride;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (const int rc = t3d_fold_fallback(a.scale, st)) return rc;      // no derive prologue here: finalize as its own launch
  const size_t lds = ((size_t)(SA_T / (C / 8)) * C + 2 * (size_t)C + R + SA_T) * sizeof(float);      // <= 48 KB
  if (dtype == T3D_F32) T3D_LAUNCH(se_after_bwd_kernel<float>, dim3(B), dim3(SA_T), lds, st, a);
  else if (dtype == T3D_BF16) T3D_LAUNCH(se_after_bwd_kernel<bf16_t>, dim3(B), dim3(SA_T), lds, st, a);
  else return T3D_ERR_ARG;
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
