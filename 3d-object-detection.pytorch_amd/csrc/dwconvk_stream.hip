// Depthwise K x K convolution forward (K = 3 or 5, stride 1 or 2), the streaming skeleton of dwconv3_stream.hip made
// generic in the stencil size, plus the per-sample channel sums squeeze-excite needs (MobileNetV3: the 5x5 layers and
// every SE block went through the LDS-tiled kernel of dwconv_fwd.hip at 0.2-0.3 TB/s).
//
// A thread owns 2 channels of NC ADJACENT output columns (round 5; one column before) and walks down a chunk of rows; no LDS, no
// barriers in the walk.  The K + (NC - 1) S input columns it loads per row feed all NC outputs: 8 loads and activations per four
// outputs of a 5x5 stride-1 layer instead of 20.  Worth 8-20 % on the stride-1 layers, nothing at stride 2 (launch_ks): the walk
// is bound by its 25 packed FMAs per output pair and by registers (222 at K = 5, NC = 4) more than by the tap loads.
// Input row `rel` (counted from the first row the chunk needs) feeds output row (rel - ky) / S for every tap row ky
// with (rel - ky) % S == 0, so at most NA = ceil(K / S) output rows are open at once.  The walk is unrolled over
// U = NA * S input rows: inside the unrolled body the open rows' accumulator slots ((rel - ky) / S mod NA), the row that
// completes ((rel - K + 1) / S) and the prefetch-ring slot are all compile-time constants.
// Zero padding applies to the ACTIVATED tensor: out-of-image columns are masked per item, out-of-image rows skipped
// (wave-uniform); loads are unconditional from clamped addresses.
#include <cstdlib>
#include <type_traits>
#include "dwconv_walk.h"

namespace {

struct DwkArgs {
  const void* x;
  void* y;
  const float* w;  // [C][K*K]
  const float *scale, *shift;
  int act;
  double* stats;
  float* gap;      // [B][C] per-sample sums of the (rounded) output, or null (int64 fixed point when gapq: common.h)
  int gapq;
  int B, H, W, C, Ho, Wo;
  int rows_per_chunk, nchunks, slab, nitems;
  int Wb;          // column blocks per row: ceil(Wo / NC)
  int nrep;
  long long rstride;
  T3dQuant quant;  // BatchNorm sums snapped onto a fixed grid: order-independent (common.h)
};

constexpr int floormod(int a, int n) { return ((a % n) + n) % n; }
constexpr int floordiv(int a, int n) { return (a - floormod(a, n)) / n; }

template <typename T, int K, int S, int NC>
__global__ __launch_bounds__(256) void dwk_fwd_kernel(const DwkArgs a) {
  constexpr int CH = 2, PAD = (K - 1) / 2, NA = (K + S - 1) / S, U = NA * S, KC = K + (NC - 1) * S;
  extern __shared__ double lstat[];  // [2][Cb] fp64: exact adds of the snapped partial sums (common.h)
  using RV = rawvec<T, CH>;
  const int CG = a.C / CH;
  int cg, ox_fixed = 0, q0, qstride;
  bool on;
  if (!a.slab) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    on = j < a.Wb * CG;
    cg = on ? j % CG : 0;
    ox_fixed = on ? j / CG : 0;
    q0 = blockIdx.y;
    qstride = gridDim.y;
  } else {
    cg = blockIdx.y * 64 + (threadIdx.x & 63);
    on = cg < CG;
    if (!on) cg = 0;
    q0 = blockIdx.x * 4 + (threadIdx.x >> 6);
    qstride = gridDim.x * 4;
  }
  const int c0 = cg * CH;
  const bool affine = a.scale != nullptr || a.act != T3D_ACT_NONE;

  f32x2 wt[K * K];     // the two channels' weights, packed
  float sc[CH], sh[CH], psum[CH], psq[CH];
#pragma unroll
  for (int t = 0; t < K * K; ++t) wt[t] = f32x2{a.w[(size_t)c0 * (K * K) + t], a.w[(size_t)(c0 + 1) * (K * K) + t]};
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    sc[i] = a.scale ? a.scale[c0 + i] : 1.f;
    sh[i] = a.scale ? a.shift[c0 + i] : 0.f;
    psum[i] = psq[i] = 0.f;
  }

  for (int q = q0; q < a.nitems && on; q += qstride) {
    int ox, rest;
    if (!a.slab) { ox = ox_fixed; rest = q; } else { ox = q % a.Wb; rest = q / a.Wb; }
    ox *= NC;                                   // first output column of this thread's block
    const int chunk = rest % a.nchunks, b = rest / a.nchunks;
    const T* __restrict__ x = reinterpret_cast<const T*>(a.x) + (size_t)b * a.H * a.W * a.C + c0;
    T* __restrict__ y = reinterpret_cast<T*>(a.y) + (size_t)b * a.Ho * a.Wo * a.C + c0;
    const int oy0 = chunk * a.rows_per_chunk, oy1 = min(a.Ho, oy0 + a.rows_per_chunk);
    const int ix0 = ox * S - PAD;
    float cm[KC];       // 0/1: column inside the image
    int coff[KC];
#pragma unroll
    for (int c = 0; c < KC; ++c) {
      cm[c] = (ix0 + c >= 0 && ix0 + c < a.W) ? 1.f : 0.f;
      coff[c] = min(max(ix0 + c, 0), a.W - 1) * a.C;
    }
    const int iy_first = oy0 * S - PAD, nrel = (oy1 - 1 - oy0) * S + K;   // input rows walked: rel = 0 .. nrel-1
    RV ring[U][KC];
    auto fetch = [&](int rel, RV* dst) {
      const T* rp = x + (size_t)min(max(iy_first + rel, 0), a.H - 1) * a.W * a.C;
#pragma unroll
      for (int c = 0; c < KC; ++c) dst[c] = *reinterpret_cast<const RV*>(rp + coff[c]);
    };
#pragma unroll
    for (int u = 0; u < U; ++u) fetch(u, ring[u]);
    f32x2 acc[NA][NC];
#pragma unroll
    for (int r = 0; r < NA; ++r)
#pragma unroll
      for (int oc = 0; oc < NC; ++oc) acc[r][oc] = f32x2{0.f, 0.f};
    float gs[CH] = {0.f, 0.f};

    for (int base = 0; base < nrel; base += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int rel = base + u;
        if (rel < nrel) {          // wave-uniform in the slab mapping, near-uniform otherwise
          const int iy = iy_first + rel;
          const float rm = (iy >= 0 && iy < a.H) ? 1.f : 0.f;
          f32x2 v[KC];
#pragma unroll
          for (int c = 0; c < KC; ++c) {
            float t[CH] = {(float)ring[u][c][0], (float)ring[u][c][1]};
            if (affine) act_affine_vec<CH>(t, sc, sh, a.act);
            const float m = cm[c] * rm;
            v[c] = f32x2{t[0] * m, t[1] * m};
          }
          fetch(rel + U, ring[u]);   // refill this slot: U rows ahead
          // scatter the row into the open output rows
#pragma unroll
          for (int ky = 0; ky < K; ++ky) {
            if (floormod(u - ky, S) == 0) {                       // compile time
              const int slot = floormod(floordiv(u - ky, S), NA); // compile time (base is a multiple of U = NA*S)
              if (rel >= ky) {                                    // output row (rel-ky)/S exists (scalar test)
#pragma unroll
                for (int oc = 0; oc < NC; ++oc)
#pragma unroll
                  for (int c = 0; c < K; ++c) acc[slot][oc] = pk_fma(v[oc * S + c], wt[ky * K + c], acc[slot][oc]);
              }
            }
          }
          // the output row whose last tap row this was
          if (floormod(u - (K - 1), S) == 0) {                    // compile time
            const int slot = floormod(floordiv(u - (K - 1), S), NA);
            if (rel >= K - 1) {
              const int oy = oy0 + (rel - (K - 1)) / S;
#pragma unroll
              for (int oc = 0; oc < NC; ++oc) {
                if (NC == 1 || ox + oc < a.Wo) {            // (the last block of a row may hold fewer columns)
                  RV o;
                  o[0] = (T)acc[slot][oc][0];
                  o[1] = (T)acc[slot][oc][1];
#pragma unroll
                  for (int i = 0; i < CH; ++i) {
                    const float r = (float)o[i];
                    psum[i] += r;
                    psq[i] = fmaf(r, r, psq[i]);
                    gs[i] += r;
                  }
                  *reinterpret_cast<RV*>(y + ((size_t)oy * a.Wo + ox + oc) * a.C) = o;
                }
              }
            }
#pragma unroll
            for (int oc = 0; oc < NC; ++oc) acc[slot][oc] = f32x2{0.f, 0.f};
          }
        }
      }
    }
    if (a.gap) {
#pragma unroll
      for (int i = 0; i < CH; ++i) t3d_pool_add(a.gap, (size_t)b * a.C + c0 + i, gs[i], a.gapq);
    }
  }  // item loop

  if (a.stats) {
    const int cbase = a.slab ? blockIdx.y * 64 * CH : 0;
    const int Cb = a.slab ? min(64 * CH, a.C - cbase) : a.C;
    for (int i = threadIdx.x; i < 2 * Cb; i += 256) lstat[i] = 0.0;
    __syncthreads();
    if (on) {
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        atomicAdd(lstat + c0 - cbase + i, t3d_snap(psum[i], a.quant, false));
        atomicAdd(lstat + Cb + c0 - cbase + i, t3d_snap(psq[i], a.quant, true));
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 2 * Cb; i += 256)
      if (lstat[i] != 0.0)
        atomicAdd(a.stats + (size_t)((blockIdx.x + blockIdx.y) % a.nrep) * a.rstride + (size_t)(i / Cb) * a.C + cbase + i % Cb,
                  lstat[i]);
  }
}

template <typename T, int K, int S, int NC>
int launch_nc(DwkArgs& a, const DwWalkPlan& plan, hipStream_t st) {
  a.Wb = cdiv(a.Wo, NC);
  const dim3 grid = dw_apply_plan(a, plan);
  // (throughput mode only, as in dwconv3_stream.hip)
  a.quant = dw_quant<T>(a.stats, (long long)a.B * a.Ho * a.Wo);
  T3D_LAUNCH_TIMED((dwk_fwd_kernel<T, K, S, NC>), grid, dim3(256), plan.lds, st, a);
  T3D_CHECK_LAUNCH();
  return T3D_OK;
}

// output columns per thread: four for stride 1 where the row has them, one for stride 2 (dwconv_walk.h: dw_rowk_fwd_spec)
template <typename T, int K, int S>
int launch_ks(DwkArgs& a, const DwShape& s, hipStream_t st) {
  const DwWalkPlan plan = dw_walk_plan(s.B, s.C, dw_rowk_fwd_spec(s));
  if constexpr (S == 1) {
    if (plan.variant == 4) return launch_nc<T, K, S, 4>(a, plan, st);
  }
  return launch_nc<T, K, S, 1>(a, plan, st);
}

template <typename T>
int launch_t(DwkArgs& a, const DwShape& s, hipStream_t st) {
  if (s.k == 5 && s.stride == 1) return launch_ks<T, 5, 1>(a, s, st);
  if (s.k == 5 && s.stride == 2) return launch_ks<T, 5, 2>(a, s, st);
  if (s.k == 3 && s.stride == 1) return launch_ks<T, 3, 1>(a, s, st);
  return launch_ks<T, 3, 2>(a, s, st);
}

}  // namespace

// T3D_DW_ROWK forward: the generic walk -- the 5x5 layers the plane and tile kernels leave, and 3x3 with squeeze-excite pooled
// sums (no SE gate on the INPUT); all three storage types (fp16: the 5x5 layers of the MobileNetV3 layouts at inference)
bool t3d_dw_rowk_fwd_can(const DwShape& s) {
  return (s.k == 3 || s.k == 5) && s.stride_1_or_2() && !s.gated && (s.f32_or_bf16() || s.dtype == T3D_F16);
}

int t3d_dw_rowk_fwd(const DwShape& s, const void* x, const t3d_prologue* pro, const float* w, void* y, double* stats,
                    float* gap_sum, hipStream_t st) {
  if (!t3d_dw_rowk_fwd_can(s)) return T3D_ERR_ARG;
  DwkArgs a{};
  a.x = x; a.y = y; a.w = w; a.stats = stats; a.gap = gap_sum; a.gapq = g_t3d_reduce.pool_exact;
  if (pro) { a.scale = pro->scale; a.shift = pro->shift; a.act = pro->act; }
  a.B = s.B; a.H = s.H; a.W = s.W; a.C = s.C;
  a.Ho = dw_out(s.H, s.k, s.stride);
  a.Wo = dw_out(s.W, s.k, s.stride);
  if (s.dtype == T3D_F32) return launch_t<float>(a, s, st);
  if (s.dtype == T3D_BF16) return launch_t<bf16_t>(a, s, st);
  return launch_t<f16_t>(a, s, st);
}
