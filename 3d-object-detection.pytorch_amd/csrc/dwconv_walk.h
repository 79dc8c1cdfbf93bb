// What the depthwise kernel files share (dwconv3_stream.hip, dwconv3_bwd_stream.hip, dwconvk_stream.hip, dwconv5_bwd_stream.hip,
// dwconv5_plane7.hip, dwconv_tile.hip):
//   device: the register-vector type, raw buffer loads / stores, the packed clamp form of ReLU6, opaque channel pairs, the
//           weight staging of the tile and plane kernels;
//   host:   ONE launch planner for the six row-walk launchers of T3D_DW_ROW3 and T3D_DW_ROWK -- a pure function from a small
//           spec to chunking, lane mapping, persistent grid, weight-gradient slot count and LDS bytes -- with the six specs
//           next to it, and the few launcher lines that read the process state (slots, snapped sums, the backward's arguments).
// t3d_dwconv_plan (dwconv_route.hip) answers from the same spec functions the launchers call.
#pragma once
#include <cstdlib>
#include <type_traits>
#include "dwconv_route.h"

namespace {

// ---- device ---------------------------------------------------------------------------------------------------------------

template <typename T, int CH> using rawvec = T __attribute__((ext_vector_type(CH)));

// raw buffer loads / stores: scalar descriptor + 32-bit scalar row offset + 32-bit lane offset -- no 64-bit vector address
// arithmetic in the row loop (20 v_lshl_add_u64 + 8 v_mul_lo_u32 per three rows of the s=1 forward before); an offset beyond
// num_records reads zeros / drops the store, which also replaces the store predicates of edge lanes
template <typename RV>
__device__ __forceinline__ RV bufload(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  if constexpr (sizeof(RV) == 4) return __builtin_bit_cast(RV, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
  else if constexpr (sizeof(RV) == 8) return __builtin_bit_cast(RV, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
  else return __builtin_bit_cast(RV, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
template <typename RV>
__device__ __forceinline__ void bufstore(const RV& v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  if constexpr (sizeof(RV) == 4) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), r, voff, soff, 0);
  else if constexpr (sizeof(RV) == 8) __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, voff, soff, 0);
  else __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, voff, soff, 0);
}

// ReLU6 of a BatchNorm affine in ONE packed instruction (bf16 storage): relu6(s x + t) = 6 clamp01((s/6) x + t/6), and
// v_pk_fma_f32 takes the clamp modifier (result clamped to [0, 1] per half; probed on the hardware with a scratch program
// that is no longer in the tree).  Forward: the caller scales (s, t) by 1/6 once per thread and folds the 6 into whatever
// multiplies the activated value next (the stencil weights): two v_med3_f32 per channel pair leave the row loop.  Backward:
// the activated operand a' = a/6 feeds the weight gradient (the 6 is applied once, when the accumulators are flushed) and
// IS the derivative mask of the own columns (0 < a' < 1).  fp32 storage keeps the exact form.
__device__ __forceinline__ f32x2 pk_fma_clamp01(f32x2 a, f32x2 b, f32x2 c) {
  f32x2 d;
  asm("v_pk_fma_f32 %0, %1, %2, %3 clamp" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}

// A channel pair as it lies in memory, kept OPAQUE until the point of use: held as a vector of two bf16 the compiler widened
// every loaded pair to two fp32 registers at once (the plane backward then wanted ~480 registers for three 49-pixel planes).
template <typename T> struct Pair;
template <> struct Pair<bf16_t> {
  typedef unsigned int raw;
  static __device__ __forceinline__ raw load(const bf16_t* p) { return *reinterpret_cast<const unsigned int*>(p); }
  static __device__ __forceinline__ f32x2 widen(raw v) { return f32x2{__uint_as_float(v << 16), __uint_as_float(v & 0xffff0000u)}; }
  static __device__ __forceinline__ void opaque(raw& v) { asm volatile("" : "+v"(v)); }
};
template <> struct Pair<float> {
  typedef f32x2 raw;
  static __device__ __forceinline__ raw load(const float* p) { return *reinterpret_cast<const f32x2*>(p); }
  static __device__ __forceinline__ f32x2 widen(raw v) { return v; }
  static __device__ __forceinline__ void opaque(raw& v) { asm volatile("" : "+v"(v)); }
};

// weights of the workgroup's channel slab -> LDS [K2][SLAB] (tap-major: a lane reads its channel pair as one 8-byte word)
template <int K2, int SLAB>
__device__ __forceinline__ void stage_weights(float* wl, const float* __restrict__ w, int cbase, int Cb) {
  for (int i = threadIdx.x; i < K2 * Cb; i += 256) {
    const int cl = i / K2, t = i - cl * K2;
    wl[t * SLAB + cl] = w[(size_t)cbase * K2 + i];
  }
}

// ---- host: the row-walk launch planner ------------------------------------------------------------------------------------
// A thread keeps CH channels (one channel group) for its whole life and walks (column, row chunk, sample) items down a chunk
// of rows.  Lanes map onto (column, group) in one of two ways:
//   flat: thread = (column, group) of the row strip (grid.x covers it), items = (sample, chunk), grid.y walks them;
//   slab: lane = group inside a 64-group slab (grid.y), items = (column, sample, chunk), the waves of grid.x walk them.
// A spec is everything in which the six launchers differ.

constexpr int kDwThreads = 256;        // (512-thread blocks measured 4-5x slower in the 3x3 backward: register budget)
constexpr int kDwAnyWaste = 100;       // waste_pct of a launcher without a waste rule

struct DwWalkSpec {
  int variant;          // the template instance the launcher takes: channels per thread, or output columns (k x k forward)
  int ch;               // channels per thread
  int rows;             // rows a column walks: output rows, or input rows where the thread owns input pixels
  int chunk_cols;       // columns that count as work when the rows are cut into chunks
  int grid_cols;        // columns (pairs, blocks) the lanes or items cover
  long long want;       // (thread, item) pairs wanted: enough to fill the chip, each chunk re-reads its halo rows
  int min_rows;         // no chunk shorter than this
  int target;           // persistent workgroups: enough to fill the chip, few enough that the per-block flush stays cheap
  int waste_pct;        // flat when the slabs would leave more than this share of their lanes idle (and below 64 groups)
  int lds_per_channel;  // bytes of dynamic LDS per channel of the workgroup's range
  bool lds_whole;       // the LDS is sized for all C channels even in the slab mapping
  bool lds_must_fit;    // a flat mapping whose scratch passes 64 KiB goes to slabs
};

struct DwWalkPlan {
  int rows_per_chunk, nchunks, slab, nitems;
  unsigned gx, gy;
  int slots_needed;     // weight-gradient slots: one per workgroup that flushes a given channel
  size_t lds;
  int variant;
};

inline DwWalkPlan dw_walk_plan(int B, int C, const DwWalkSpec& s) {
  DwWalkPlan p{};
  p.variant = s.variant;
  const int CG = C / s.ch, ns = cdiv(CG, 64), slab_lanes = ns * 64;
  const long long chunk_row = (long long)B * s.chunk_cols * CG;
  int nchunks = (int)((s.want + chunk_row - 1) / chunk_row);
  const int max_chunks = s.rows / s.min_rows < 1 ? 1 : s.rows / s.min_rows;
  if (nchunks > max_chunks) nchunks = max_chunks;
  if (nchunks < 1) nchunks = 1;
  p.rows_per_chunk = cdiv(s.rows, nchunks);
  p.nchunks = cdiv(s.rows, p.rows_per_chunk);
  bool flat = CG < 64 || (slab_lanes - CG) * 100 > s.waste_pct * slab_lanes;
  if (flat && CG >= 64 && s.lds_must_fit && (size_t)s.lds_per_channel * C > 64 * 1024) flat = false;
  p.slab = !flat;
  if (flat) {
    p.nitems = B * p.nchunks;
    const int jb = cdiv(s.grid_cols * CG, kDwThreads);
    int gy = s.target / jb;
    if (gy > p.nitems) gy = p.nitems;
    if (gy < 1) gy = 1;
    p.gx = jb; p.gy = gy;
    p.slots_needed = jb * gy;
  } else {
    p.nitems = s.grid_cols * B * p.nchunks;
    int gx = s.target / ns;
    if (gx > cdiv(p.nitems, kDwThreads / 64)) gx = cdiv(p.nitems, kDwThreads / 64);
    if (gx < 1) gx = 1;
    p.gx = gx; p.gy = ns;
    p.slots_needed = gx;
  }
  p.lds = (size_t)s.lds_per_channel * ((p.slab && !s.lds_whole) ? 64 * s.ch : C);
  return p;
}

inline int dw_out(int n, int k, int stride) { return (n + 2 * ((k - 1) / 2) - k) / stride + 1; }

// 3x3 forward (dwconv3_stream.hip).  Stride 1 walks column PAIRS while the input stays below 2 GB (32-bit buffer offsets), but
// its chunks are still counted in columns.  Persistent blocks, from a sweep whose script is no longer in the tree: the
// small-spatial s=1 layers gain 4-5 % at 768 (28x28x192 38.0 -> 35.7 us, 14x14x384 24.8 -> 23.7).
inline bool dw_row3_fwd_pairs(const DwShape& s) { return s.stride == 1 && s.bytes() < (1ull << 31); }
inline DwWalkSpec dw_row3_fwd_spec(const DwShape& s) {
  const int Ho = dw_out(s.H, 3, s.stride), Wo = dw_out(s.W, 3, s.stride);
  return {4, 4, Ho, Wo, dw_row3_fwd_pairs(s) ? (Wo + 1) / 2 : Wo, 256LL * 64 * 40, 8, (s.stride == 1 && s.H > 28) ? 512 : 768,
          kDwAnyWaste, 2 * (int)sizeof(double), true, false};
}

// 3x3 backward, stride 1 (dwconv3_bwd_stream.hip): column pairs.  2 channels per thread: half the live registers (no AGPR
// spills, twice the resident waves) beats the wider loads of 4 channels per thread by 5-30 % on every layer.  From a sweep
// whose script is no longer in the tree: the 4-channel variant needs AGPR spill space (1 wave/SIMD) and is best with one
// block per CU; the 2-channel variant fits 2 waves/SIMD and is best with two (every extra block is one more flush).
// Slabs only when they waste < 12 % of the lanes (14x14x576 -- 288 channel pairs, 5 slabs -- is 5 % faster in slabs than
// flattened, where every workgroup flushes sums of up to 512 channels instead of 128).
// LDS: [11][Cb] fp64 reduction scratch (before it: [9][Cb] weights, [3][Cb] derived coefficients).
inline DwWalkSpec dw_row3_bwd_s1_spec(const DwShape& s) {
  const int ch = s.C % 2 == 0 ? 2 : 4, Wp = (s.W + 1) / 2;
  return {ch, ch, s.H, Wp, Wp, 256LL * 64 * 24, 8, ch == 2 ? 512 : 256, 12, 22 * (int)sizeof(float), false, false};
}

// 3x3 backward, stride 2: a thread owns an output column and its 2x2 input pixels
// (round 4 sweep: 14x14x576 46.6 -> 41.4 us, 28x28x192 54.3 -> 51.5 at 512 blocks against 384)
inline DwWalkSpec dw_row3_bwd_s2_spec(const DwShape& s) {
  const int Ho = dw_out(s.H, 3, 2), Wo = dw_out(s.W, 3, 2);
  return {4, 4, Ho, Wo, Wo, 256LL * 64 * 24, 4, 512, kDwAnyWaste, 22 * (int)sizeof(float), false, false};
}

// k x k forward (dwconvk_stream.hip): NC adjacent output columns per thread.  Measured per layer of mobilenetv3_large at
// B = 256 (the timing script is no longer in the tree; us at NC = 1 / 2 / 4):
//   3x3 s1 14^2 x 480 / 672 (squeeze-excite): 62.6 / 50.1 / 49.2 and 77.9 / 61.4 / 57.3;  5x5 s1 28^2 x 120: 93.7 / 105.7 / 77.8,
//   7^2 x 960: 66.3 / 78.6 / 62.8;  5x5 s2 56^2 x 72: 93.1 / 95.3 (/ 93.8 at NC = 2), 14^2 x 672: 69.2 / 84.9 -- four columns for
//   stride 1, one for stride 2.
// Row chunks per image: enough (thread, item) pairs to fill the chip once (~1600 waves) and no more -- every chunk re-reads
// K - 1 halo rows and pays the ring fill again.  (Round 6, isolated at B = 256: 28x28x120 5x5 s1 with four columns per
// thread ran 79 us in three chunks, 58 in one; the 40-fold target dates from the one-column kernel.)
inline DwWalkSpec dw_rowk_fwd_spec(const DwShape& s) {
  const int Ho = dw_out(s.H, s.k, s.stride), Wo = dw_out(s.W, s.k, s.stride);
  const int nc = (s.stride == 1 && Wo >= 4) ? 4 : 1, Wb = cdiv(Wo, nc);
  const bool k5s1 = s.k == 5 && s.stride == 1;
  return {nc, 2, Ho, Wb, Wb, (k5s1 && nc > 1) ? 256LL * 64 * 6 : 256LL * 64 * 40, 8, k5s1 ? 1024 : 768, 8,
          2 * (int)sizeof(double), false, false};
}

// 5x5 backward (dwconv5_bwd_stream.hip).  Stride 1: every chunk re-reads 4 halo rows of the gradient.  LDS: [27][Cb] fp64,
// 27 KB for a slab; a flat mapping has fewer than 128 channels or fits 64 KiB -- the reduction scratch must fit LDS.
inline DwWalkSpec dw_rowk_bwd_s1_spec(const DwShape& s) {
  return {2, 2, s.H, s.W, s.W, 256LL * 64 * 24, 5, 512, 8, 54 * (int)sizeof(float), false, true};
}
inline DwWalkSpec dw_rowk_bwd_s2_spec(const DwShape& s) {
  const int Ho = dw_out(s.H, 5, 2), Wo = dw_out(s.W, 5, 2);
  return {2, 2, Ho, Wo, Wo, 256LL * 64 * 24, 4, 512, 8, 54 * (int)sizeof(float), false, true};
}

// the spec of a call that routes to T3D_DW_ROW3 or T3D_DW_ROWK
inline DwWalkSpec dw_walk_spec(int route, const DwShape& s) {
  if (route == T3D_DW_ROW3)
    return !s.backward ? dw_row3_fwd_spec(s) : (s.stride == 2 ? dw_row3_bwd_s2_spec(s) : dw_row3_bwd_s1_spec(s));
  return !s.backward ? dw_rowk_fwd_spec(s) : (s.stride == 2 ? dw_rowk_bwd_s2_spec(s) : dw_rowk_bwd_s1_spec(s));
}

// ---- host: launcher lines that read the process state -------------------------------------------------------------------------

// the plan's geometry into a row-walk argument struct; reduction replicas as set for the process
template <class A>
inline dim3 dw_apply_plan(A& a, const DwWalkPlan& p) {
  a.rows_per_chunk = p.rows_per_chunk; a.nchunks = p.nchunks; a.slab = p.slab; a.nitems = p.nitems;
  a.nrep = g_t3d_reduce.nrep;
  a.rstride = g_t3d_reduce.stats_stride;
  return dim3(p.gx, p.gy);
}

// depthwise weight gradient: one slot per workgroup when the caller provides enough of them (t3d_set_dw_slots)
template <class A>
inline void dw_take_slots(A& a, int needed) {
  a.dw_slots = (a.dw && g_t3d_reduce.dw_slots >= needed) ? needed : 0;
  a.dw_used = a.dw ? g_t3d_reduce.dw_used : nullptr;
}

// BatchNorm sums snapped onto a fixed grid (common.h).  Throughput mode only: in fp32 storage the sums' order noise stays at
// 1e-6 of the outputs and the grid would be one more perturbation between the parity mode and the reference.
template <typename T>
inline T3dQuant dw_quant(const double* stats, long long count) {
  return (stats && std::is_same<T, bf16_t>::value && !T3D_ENV_SET("T3D_NO_SNAP")) ? t3d_quant_for(count) : T3dQuant{0.0, 0.0};
}

// what both row-walk backward entry points take from the call
template <class A>
inline void dw_fill_bwd(A& a, const DwShape& s, const void* dz, const void* y, const t3d_bnbwd* bb, const float* w, const void* x,
                        const t3d_prologue* pro, const void* residual, void* dx, double* stats, float* dw) {
  a.dz = dz; a.y = y; a.x = x; a.res = residual; a.dx = dx; a.w = w;
  a.alpha = bb->alpha; a.beta = bb->beta; a.gamma = bb->gamma; a.per_sample = bb->per_sample;
  if (pro) { a.scale = pro->scale; a.shift = pro->shift; a.act = pro->act; }
  a.stats = stats; a.dw = dw;
  a.B = s.B; a.H = s.H; a.W = s.W; a.C = s.C;
}

}  // namespace
