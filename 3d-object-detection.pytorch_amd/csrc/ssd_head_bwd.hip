// Backward of the SSD heads' `ReLU(BN(y)) -> 1x1 conv + bias` half (the SSDHead of configs/detection/mnv2_ssd_300_2_heads.py
// :15-37 of the reference, trained by its optimizer :145-153), every head of the detector in ONE call of TWO launches:
//   shb_pass_kernel    a workgroup per (head, 128 rows): the data gradient g = (do . W) (.) [fmaf(scale, y, shift) > 0], and the
//                      workgroup's partial sums of dW = do^T relu(.), of the bias gradient and of sum(g), sum(g*y);
//   shb_finish_kernel  adds the partials of every output element over a fixed tree (fp64) and writes dW, dbias, stats.
// `do` is the MultiBox loss's fp32 gradient (t3d_ssd_multibox_loss) and is never rounded: t3d_pwconv_dgrad / _wgrad take it in
// the storage dtype, which for gradients already divided by avg = max(sum num_pos, 1) is not acceptable.  A head has at most
// 64 output channels, so a lane keeps one column of W and one column of dW in registers and the three products share one pass
// over `do` and `y`.
// Arithmetic: the dot product behind g runs in fp64 (a product of two fp32 numbers is exact there), so that g is the exact
// result rounded ONCE to the storage dtype; dW accumulates in fp32 over the workgroup's rows and in fp64 across workgroups;
// the bias gradient and the BatchNorm-backward sums are fp64 throughout.
// Determinism: no floating-point atomics -- a lane adds its rows in ascending order, the four waves are combined in wave
// order, the workgroups over a fixed tree of their indices (as the engine's `_flush_dw` does for the depthwise slots).
// Plain vector code: the fp32 matrix instructions run at the vector rate on gfx950 and have no fp64-accumulating fp32-input
// form.  Measured at batch 80 (bf16, the four real heads): 0.31 ms for the call.  The pass holds a W
// column (128 VGPRs as doubles) and a dW column (64) per lane, runs at ONE wave per SIMD and waits out every row's scalar and
// y loads: it is latency-bound, an order of magnitude above its fp64 issue time.  Asking for two waves per SIMD spilled to
// scratch; loading the next row's y ahead measured slower (0.37 ms).  Open.
#include <climits>

#include "common.h"

namespace {

constexpr int kMaxHeads = 8;
constexpr int kNT = 256, kNW = kNT / 64;
constexpr int kRows = 128;       // rows of a workgroup
constexpr int kMaxN = 64;

struct ShbHead {
  const float* dout;     // [M][ns]
  const void* y;         // [M][C]
  const float *scale, *shift;
  const void* w;         // [ns][C]
  void* g;               // [M][C]
  double* stats;         // [2C] +=
  float* dW;             // [n][C]
  float* dbias;          // [n]
  double* stpart;        // [tiles][2][C]
  double* dbpart;        // [tiles][n]
  float* dwpart;         // [tiles][n][C]
  int M, C, n, ns, tiles, tile0, fin0, act;
};

struct ShbArgs {
  ShbHead h[kMaxHeads];
  int nheads;
};

__device__ __forceinline__ float ldw(const float* p, size_t i) { return p[i]; }
__device__ __forceinline__ float ldw(const bf16_t* p, size_t i) { return (float)p[i]; }

// double -> fp32 with round-to-odd: the bf16 rounding that follows is then the single rounding of the fp64 value
__device__ __forceinline__ float f64_to_f32_odd(double x) {
  float f = (float)x;
  const double d = (double)f;
  if (d != x) {
    unsigned b = __float_as_uint(f);
    if (!(b & 1u)) f = __uint_as_float(fabs(d) < fabs(x) ? b + 1u : b - 1u);
  }
  return f;
}
__device__ __forceinline__ void stg(float* p, size_t i, double v) { p[i] = (float)v; }
__device__ __forceinline__ void stg(bf16_t* p, size_t i, double v) { p[i] = (bf16_t)f64_to_f32_odd(v); }

// LDS plan of a workgroup (bytes): red [kMaxN][64] fp32 | sred [kNW][2][64] fp64
constexpr int kLds = kMaxN * 64 * 4 + kNW * 2 * 64 * 8;

// A wave walks rows; its lanes are 64 consecutive channels.  A row's `do` values are the same for every lane, so they come
// through the SCALAR cache and enter the arithmetic as scalar operands: the row index is wave-uniform, and `dout` -- written
// by an earlier launch, read-only in this one -- is addressed as constant memory, which is what makes hipcc select s_load
// for it next to the stores to g (as plain global memory it became 16 vector loads of one address per row; a version that
// staged the rows in LDS read them back with 48 broadcast 16-byte reads per row).  NS == ns exactly: whole 32-byte pieces.
typedef const float __attribute__((address_space(4))) * shb_cptr;
template <typename T, int NS>
__device__ __forceinline__ void shb_tile(const ShbHead& h, int tile, unsigned char* smem, const float* __restrict__ dout,
                                         const T* __restrict__ yp, const T* __restrict__ wp, T* __restrict__ gp,
                                         float* __restrict__ dwpart, double* __restrict__ stpart, double* __restrict__ dbpart) {
  float* red = reinterpret_cast<float*>(smem);
  double* sred = reinterpret_cast<double*>(red + kMaxN * 64);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int M = h.M, C = h.C, n = h.n;
  const int row_lo = tile * kRows;
  const int row_hi = min(row_lo + kRows, M);
  if (tid < n) {                                     // the tile's column sums of do, rows ascending
    double db = 0.0;
    for (int r = row_lo; r < row_hi; ++r) db += (double)dout[(size_t)r * NS + tid];
    dbpart[(size_t)tile * n + tid] = db;
  }
  for (int cbase = 0; cbase < C; cbase += 64) {
    const int c = cbase + lane;
    const bool live = c < C;
    double wd[NS];
    float acc[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      wd[j] = (live && j < n) ? (double)ldw(wp, (size_t)j * C + c) : 0.0;
      acc[j] = 0.f;
    }
    const float sc = live ? h.scale[c] : 0.f, sh = live ? h.shift[c] : 0.f;
    const bool relu = h.act == T3D_ACT_RELU;
    double sg = 0.0, sgy = 0.0;
    for (int r = row_lo + wv; r < row_hi; r += kNW) {       // (wave-uniform)
      const shb_cptr dr = (shb_cptr)(dout + (size_t)r * NS);
      float d[NS];
#pragma unroll
      for (int j = 0; j < NS; ++j) d[j] = dr[j];
      double ga = 0.0;
#pragma unroll
      for (int j = 0; j < NS; ++j) ga = fma((double)d[j], wd[j], ga);
      if (live) {
        const size_t idx = (size_t)r * C + c;
        const float yv = ldw(yp, idx);
        const float u = fmaf(yv, sc, sh);
        const bool pos = relu ? u > 0.f : true;
        const double gv = pos ? ga : 0.0;
        const float a = pos ? u : 0.f;
        stg(gp, idx, gv);
        sg += gv;
        sgy = fma(gv, (double)yv, sgy);
#pragma unroll
        for (int j = 0; j < NS; ++j) acc[j] = fmaf(d[j], a, acc[j]);
      }
    }
    // the four waves' partials, in wave order
    __syncthreads();                                 // (the previous channels' readers of red / sred are done)
    sred[(wv * 2 + 0) * 64 + lane] = sg;
    sred[(wv * 2 + 1) * 64 + lane] = sgy;
    for (int w = 0; w < kNW; ++w) {
      if (wv == w) {
        if (w == 0) {
#pragma unroll
          for (int j = 0; j < NS; ++j) red[j * 64 + lane] = acc[j];
        } else if (w < kNW - 1) {
#pragma unroll
          for (int j = 0; j < NS; ++j) red[j * 64 + lane] += acc[j];
        } else if (live) {
          float* dst = dwpart + (size_t)tile * n * C + c;
#pragma unroll
          for (int j = 0; j < NS; ++j)
            if (j < n) dst[(size_t)j * C] = red[j * 64 + lane] + acc[j];
        }
      }
      __syncthreads();
    }
    if (wv == 0 && live) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int w = 0; w < kNW; ++w) { s0 += sred[(w * 2 + 0) * 64 + lane]; s1 += sred[(w * 2 + 1) * 64 + lane]; }
      stpart[(size_t)tile * 2 * C + c] = s0;
      stpart[(size_t)tile * 2 * C + C + c] = s1;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kNT) void shb_pass_kernel(const ShbArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int hi = 0;
  for (int i = 1; i < a.nheads; ++i)
    if ((int)blockIdx.x >= a.h[i].tile0) hi = i;     // (tile0 ascends; heads without rows share their successor's)
  const ShbHead& h = a.h[hi];
  const int tile = (int)blockIdx.x - h.tile0;
  if (tile >= h.tiles) return;
#define T3D_SHB(NS)                                                                                                     \
  case NS / 8:                                                                                                          \
    shb_tile<T, NS>(h, tile, smem, h.dout, reinterpret_cast<const T*>(h.y), reinterpret_cast<const T*>(h.w),            \
                    reinterpret_cast<T*>(h.g), h.dwpart, h.stpart, h.dbpart);                                           \
    break
  switch (h.ns >> 3) {
    T3D_SHB(8); T3D_SHB(16); T3D_SHB(24); T3D_SHB(32); T3D_SHB(40); T3D_SHB(48); T3D_SHB(56); T3D_SHB(64);
    default: break;
  }
#undef T3D_SHB
}

// Every `kFinParts`-th partial of one output element, ascending, four loads in flight (one thread walking all the
// workgroups' partials of its element was a chain of 226 memory latencies at batch 80: the call took 0.37 ms, now 0.31).
constexpr int kFinParts = 8, kFinElems = 256 / kFinParts;
template <typename P>
__device__ __forceinline__ double shb_part_sum(const P* __restrict__ src, size_t stride, int tiles, int p) {
  double s = 0.0;
  int t = p;
  for (; t + 3 * kFinParts < tiles; t += 4 * kFinParts) {
    const P x0 = src[(size_t)t * stride], x1 = src[(size_t)(t + kFinParts) * stride];
    const P x2 = src[(size_t)(t + 2 * kFinParts) * stride], x3 = src[(size_t)(t + 3 * kFinParts) * stride];
    s += (double)x0; s += (double)x1; s += (double)x2; s += (double)x3;
  }
  for (; t < tiles; t += kFinParts) s += (double)src[(size_t)t * stride];
  return s;
}

// 32 output elements of a head per workgroup -- [n*C] dW | [2C] stats | [n] dbias --, each summed by 8 threads over the
// workgroups' partials (thread p: partials p, p + 8, ...), the 8 sums then added in order of p: a fixed tree, in fp64
__global__ __launch_bounds__(256) void shb_finish_kernel(const ShbArgs a) {
  __shared__ double part[kFinParts][kFinElems];
  int hi = 0;
  for (int i = 1; i < a.nheads; ++i)
    if ((int)blockIdx.x >= a.h[i].fin0) hi = i;
  const ShbHead& h = a.h[hi];
  const int el = threadIdx.x % kFinElems, p = threadIdx.x / kFinElems;
  const long long e = (long long)((int)blockIdx.x - h.fin0) * kFinElems + el;
  const long long nw = (long long)h.n * h.C, ns = 2 * h.C;
  const int kind = e < nw ? 0 : (e < nw + ns ? 1 : (e < nw + ns + h.n ? 2 : 3));
  double s = 0.0;
  if (kind == 0) s = shb_part_sum(h.dwpart + e, (size_t)nw, h.tiles, p);
  else if (kind == 1) s = shb_part_sum(h.stpart + (e - nw), (size_t)ns, h.tiles, p);
  else if (kind == 2) s = shb_part_sum(h.dbpart + (e - nw - ns), (size_t)h.n, h.tiles, p);
  part[p][el] = s;
  __syncthreads();
  if (p != 0 || kind == 3) return;
  double tot = 0.0;
#pragma unroll
  for (int q = 0; q < kFinParts; ++q) tot += part[q][el];
  if (kind == 0) h.dW[e] = (float)tot;
  else if (kind == 1) h.stats[e - nw] += tot;
  else h.dbias[e - nw - ns] = (float)tot;
}

inline bool misaligned(const void* p, uintptr_t n) { return (reinterpret_cast<uintptr_t>(p) & (n - 1)) != 0; }

// T3D_OK, or the error a call with this head would return
inline int shape_rc(int M, int C, int n, int ns) {
  if (M < 0 || C <= 0 || n < 1 || ns < 1 || n > ns) return T3D_ERR_ARG;
  if ((C % 8) || C > 1024 || ns > kMaxN || (ns % 8)) return T3D_ERR_UNSUPPORTED;
  return T3D_OK;
}

inline long long head_bytes(int M, int C, int n) {
  const long long tiles = (M + kRows - 1) / kRows;
  const long long b = tiles * (2ll * C * 8 + (long long)n * 8 + (long long)n * C * 4);
  return (b + 15) / 16 * 16;
}

}  // namespace

// include/t3d.h
extern "C" int t3d_ssd_head_bwd_work_bytes(int nheads, const int* M, const int* C, const int* n) {
  if (nheads < 0 || (nheads > 0 && (!M || !C || !n))) return T3D_ERR_ARG;
  if (nheads > kMaxHeads) return T3D_ERR_UNSUPPORTED;
  long long tot = 16;
  for (int i = 0; i < nheads; ++i) {
    if (M[i] < 0 || C[i] <= 0 || n[i] < 1) return T3D_ERR_ARG;
    if (C[i] > 1024 || n[i] > kMaxN) return T3D_ERR_UNSUPPORTED;
    tot += head_bytes(M[i], C[i], n[i]);
  }
  return tot > INT_MAX ? T3D_ERR_UNSUPPORTED : (int)tot;
}

extern "C" int t3d_ssd_head_bwd(int dtype, int nheads, const void* const* dout, const void* const* y, const void* const* scale,
                                const void* const* shift, const void* const* w, const int* M, const int* C, const int* n,
                                const int* ns, int act, void* const* g, void* const* stats, void* const* dW,
                                void* const* dbias, void* work, long long work_bytes, void* stream) {
  if (nheads < 0) return T3D_ERR_ARG;
  if (nheads == 0) return T3D_OK;
  if (!dout || !y || !scale || !shift || !w || !M || !C || !n || !ns || !g || !stats || !dW || !dbias) return T3D_ERR_ARG;
  if (act != T3D_ACT_RELU && act != T3D_ACT_NONE) return T3D_ERR_UNSUPPORTED;
  if (dtype == T3D_F16) return T3D_ERR_UNSUPPORTED;
  if (dtype != T3D_F32 && dtype != T3D_BF16) return T3D_ERR_ARG;
  if (nheads > kMaxHeads) return T3D_ERR_UNSUPPORTED;
  ShbArgs a{};
  a.nheads = nheads;
  long long rows = 0, tiles = 0, fin = 0, off = 0;
  for (int i = 0; i < nheads; ++i) {
    if (const int rc = shape_rc(M[i], C[i], n[i], ns[i])) return rc;
    if (!dout[i] || !y[i] || !scale[i] || !shift[i] || !w[i] || !g[i] || !stats[i] || !dW[i] || !dbias[i]) return T3D_ERR_ARG;
    if (misaligned(dout[i], 16) || misaligned(y[i], 4) || misaligned(w[i], 4) || misaligned(g[i], 4) || misaligned(scale[i], 4) ||
        misaligned(shift[i], 4) || misaligned(stats[i], 8) || misaligned(dW[i], 4) || misaligned(dbias[i], 4))
      return T3D_ERR_ARG;
    ShbHead& h = a.h[i];
    h.dout = static_cast<const float*>(dout[i]); h.y = y[i];
    h.scale = static_cast<const float*>(scale[i]); h.shift = static_cast<const float*>(shift[i]);
    h.w = w[i]; h.g = g[i];
    h.stats = static_cast<double*>(stats[i]); h.dW = static_cast<float*>(dW[i]); h.dbias = static_cast<float*>(dbias[i]);
    h.M = M[i]; h.C = C[i]; h.n = n[i]; h.ns = ns[i]; h.act = act;
    h.tiles = (M[i] + kRows - 1) / kRows;
    h.tile0 = (int)tiles;
    h.fin0 = (int)fin;
    // the head's partials: [tiles][2][C] fp64 | [tiles][n] fp64 | [tiles][n][C] fp32
    unsigned char* base = static_cast<unsigned char*>(work) + off;
    h.stpart = reinterpret_cast<double*>(base);
    h.dbpart = h.stpart + (size_t)h.tiles * 2 * C[i];
    h.dwpart = reinterpret_cast<float*>(h.dbpart + (size_t)h.tiles * n[i]);
    off += head_bytes(M[i], C[i], n[i]);
    rows += M[i];
    tiles += h.tiles;
    fin += ((long long)n[i] * C[i] + 2 * C[i] + n[i] + kFinElems - 1) / kFinElems;
    if (tiles > INT_MAX / 2 || (long long)M[i] * C[i] >= (1ll << 40)) return T3D_ERR_UNSUPPORTED;
  }
  if (rows == 0) return T3D_OK;
  if (!work || misaligned(work, 16) || work_bytes < off) return T3D_ERR_ARG;
  if (t3d_max_lds(dtype == T3D_F32 ? (const void*)shb_pass_kernel<float> : (const void*)shb_pass_kernel<bf16_t>, kLds) != hipSuccess)
    return T3D_ERR_UNSUPPORTED;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (dtype == T3D_F32) T3D_LAUNCH(shb_pass_kernel<float>, dim3((unsigned)tiles), dim3(kNT), kLds, st, a);
  else T3D_LAUNCH(shb_pass_kernel<bf16_t>, dim3((unsigned)tiles), dim3(kNT), kLds, st, a);
  T3D_CHECK_LAUNCH();
  T3D_LAUNCH(shb_finish_kernel, dim3((unsigned)fin), dim3(256), 0, st, a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}
