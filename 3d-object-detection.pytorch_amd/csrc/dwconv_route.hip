// Depthwise convolution entry points: validate, pick the kernel family ONCE by a pure function of the call's shape, settle
// the pending BatchNorm finalize, launch (dwconv_route.h).  Host code only.
#include "dwconv_walk.h"

namespace {

int g_forced = T3D_DW_AUTO;   // t3d_dwconv_force_route

struct Family {
  bool (*can)(const DwShape&);
  bool (*wanted)(const DwShape&);   // null: wherever it can
};
// indexed by route id
const Family kFwd[] = {{t3d_dw_tile_can, t3d_dw_tile_wanted}, {t3d_dw_row3_fwd_can, nullptr}, {t3d_dw_plane7_can, nullptr},
                       {t3d_dw_rowk_fwd_can, nullptr}, {t3d_dw_lds_can, nullptr}};
const Family kBwd[] = {{t3d_dw_tile_can, t3d_dw_tile_wanted}, {t3d_dw_row3_bwd_can, nullptr}, {t3d_dw_plane7_can, nullptr},
                       {t3d_dw_rowk_bwd_can, nullptr}, {t3d_dw_lds_can, nullptr}};
// automatic routing takes the first family of this list that can and is wanted: the specialised kernels in front of the
// general ones (plane kernel and tiles: 5x5 and small pooled 3x3 planes; 3x3 row walk; k x k row walk; LDS tiles)
const int kOrder[] = {T3D_DW_PLANE7, T3D_DW_TILE, T3D_DW_ROW3, T3D_DW_ROWK, T3D_DW_LDS};

}  // namespace

int t3d_dw_route(const DwShape& s) {
  if (s.B <= 0 || s.H <= 0 || s.W <= 0 || s.C <= 0 || (s.C % 8)) return T3D_ERR_ARG;
  if (s.backward && s.gated) return T3D_ERR_UNSUPPORTED;   // no SE gate ever precedes a depthwise conv in a training graph
  const Family* fam = s.backward ? kBwd : kFwd;
  if (g_forced != T3D_DW_AUTO) return fam[g_forced].can(s) ? g_forced : T3D_ERR_UNSUPPORTED;
  for (const int r : kOrder)
    if (fam[r].can(s) && (!fam[r].wanted || fam[r].wanted(s))) return r;
  return s.f32_or_bf16() ? T3D_ERR_UNSUPPORTED : T3D_ERR_ARG;   // (fp16 is inference forward only, and never gated)
}

extern "C" int t3d_dwconv_route(int backward, int dtype, int gated_input, int pooled, int B, int H, int W, int C, int k,
                                int stride) {
  return t3d_dw_route(DwShape{backward != 0, dtype, gated_input != 0, pooled != 0 && !backward, B, H, W, C, k, stride});
}

// the launch geometry of a row-walk call, from the spec functions its launcher calls (dwconv_walk.h); zeros for the other families
extern "C" int t3d_dwconv_plan(int backward, int dtype, int gated_input, int pooled, int B, int H, int W, int C, int k,
                               int stride, int* out) {
  if (!out) return T3D_ERR_ARG;
  const DwShape s{backward != 0, dtype, gated_input != 0, pooled != 0 && !backward, B, H, W, C, k, stride};
  const int route = t3d_dw_route(s);
  for (int i = 0; i < 9; ++i) out[i] = 0;
  if (route == T3D_DW_ROW3 || route == T3D_DW_ROWK) {
    const DwWalkPlan p = dw_walk_plan(s.B, s.C, dw_walk_spec(route, s));
    const int v[9] = {p.rows_per_chunk, p.nchunks, p.slab, p.nitems, (int)p.gx, (int)p.gy, p.slots_needed, (int)p.lds, p.variant};
    for (int i = 0; i < 9; ++i) out[i] = v[i];
  }
  return route;
}

extern "C" int t3d_dwconv_force_route(int route) {
  if (route != T3D_DW_AUTO && (route < 0 || route > T3D_DW_LDS)) return T3D_ERR_ARG;
  g_forced = route;
  return T3D_OK;
}

// The finalize rule, here and nowhere else: the 3x3 row-walk kernels derive a pending BatchNorm finalize of the coefficients
// they read in their own prologue (t3d_take_fold in their launchers; backward: shared coefficients only) -- for every other
// route the request becomes a launch of its own in front of the kernel.
extern "C" int t3d_dwconv_fwd(int dtype, const void* x, const t3d_prologue* pro, const float* w, void* y, double* stats,
                              float* gap_sum, int B, int H, int W, int C, int k, int stride, void* stream) {
  if (!x || !w || !y) return T3D_ERR_ARG;
  const DwShape s{0, dtype, pro && pro->se, gap_sum != nullptr, B, H, W, C, k, stride};
  const int route = t3d_dw_route(s);
  if (route < 0) return route;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (pro && route != T3D_DW_ROW3)
    if (const int rc = t3d_fold_fallback(pro->scale, st)) return rc;
  switch (route) {
    case T3D_DW_TILE: return t3d_dw_tile_fwd(s, x, pro, w, y, stats, gap_sum, st);
    case T3D_DW_ROW3: return t3d_dw_row3_fwd(s, x, pro, w, y, stats, gap_sum, st);
    case T3D_DW_PLANE7: return t3d_dw_plane7_fwd(s, x, pro, w, y, stats, gap_sum, st);
    case T3D_DW_ROWK: return t3d_dw_rowk_fwd(s, x, pro, w, y, stats, gap_sum, st);
    default: return t3d_dw_lds_fwd(s, x, pro, w, y, stats, gap_sum, st);
  }
}

extern "C" int t3d_dwconv_bwd(int dtype, const void* dz, const void* y, const t3d_bnbwd* bb, const float* w, const void* x,
                              const t3d_prologue* pro, const void* residual, void* dx, double* stats, float* dw, int B,
                              int H, int W, int C, int k, int stride, void* stream) {
  if (!dz || !y || !bb || !w || !x || !dx) return T3D_ERR_ARG;
  const DwShape s{1, dtype, pro && pro->se, 0, B, H, W, C, k, stride};
  const int route = t3d_dw_route(s);
  if (route < 0) return route;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (route != T3D_DW_ROW3 || bb->per_sample)
    if (const int rc = t3d_fold_fallback(bb->alpha, st)) return rc;
  switch (route) {
    case T3D_DW_TILE: return t3d_dw_tile_bwd(s, dz, y, bb, w, x, pro, residual, dx, stats, dw, st);
    case T3D_DW_ROW3: return t3d_dw_row3_bwd(s, dz, y, bb, w, x, pro, residual, dx, stats, dw, st);
    case T3D_DW_PLANE7: return t3d_dw_plane7_bwd(s, dz, y, bb, w, x, pro, residual, dx, stats, dw, st);
    case T3D_DW_ROWK: return t3d_dw_rowk_bwd(s, dz, y, bb, w, x, pro, residual, dx, stats, dw, st);
    default: return t3d_dw_lds_bwd(s, dz, y, bb, w, x, pro, residual, dx, stats, dw, st);
  }
}
