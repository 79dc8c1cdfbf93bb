// Depthwise dispatch (dwconv_route.hip): t3d_dwconv_fwd / t3d_dwconv_bwd pick ONE kernel family from the call's shape, settle
// a pending BatchNorm finalize and call that family's launcher -- a call that returns an error has launched nothing and
// consumed nothing.  Every family answers two questions next to its launcher:
//   can:    the shape, dtype and option limits its kernels are correct for (a forced route asks only this);
//   wanted: where it measured faster than the families behind it, with the timing table beside it.  Only the register
//           tiles have planes they can take and lose on; every other family is wanted wherever it can.
// A launcher called with a shape its `can` rejects returns T3D_ERR_ARG: it never answers "try the next one".
// What the kernel files share below the dispatch -- device helpers, the row-walk launch planner -- is dwconv_walk.h.
#pragma once
#include "common.h"

struct DwShape {
  int backward, dtype;
  int gated;    // squeeze-excite gate in the input prologue (pro->se)
  int pooled;   // forward: per-sample pooled sums wanted (gap_sum)
  int B, H, W, C, k, stride;
  bool f32_or_bf16() const { return dtype == T3D_F32 || dtype == T3D_BF16; }
  bool stride_1_or_2() const { return stride == 1 || stride == 2; }
  unsigned long long bytes() const { return (unsigned long long)B * H * W * C * (dtype == T3D_F32 ? 4 : 2); }   // the input tensor
};

// route id (include/t3d.h: T3D_DW_*) or the negative error code of the entry point; makes no HIP call
int t3d_dw_route(const DwShape& s);

#define T3D_DW_FWD(name)                                                                                                       \
  int name(const DwShape& s, const void* x, const t3d_prologue* pro, const float* w, void* y, double* stats, float* gap_sum, \
           hipStream_t st)
#define T3D_DW_BWD(name)                                                                                                       \
  int name(const DwShape& s, const void* dz, const void* y, const t3d_bnbwd* bb, const float* w, const void* x,              \
           const t3d_prologue* pro, const void* residual, void* dx, double* stats, float* dw, hipStream_t st)

// T3D_DW_TILE: dwconv_tile.hip
bool t3d_dw_tile_can(const DwShape& s);
bool t3d_dw_tile_wanted(const DwShape& s);
T3D_DW_FWD(t3d_dw_tile_fwd);
T3D_DW_BWD(t3d_dw_tile_bwd);
// T3D_DW_ROW3: dwconv3_stream.hip, dwconv3_bwd_stream.hip
bool t3d_dw_row3_fwd_can(const DwShape& s);
bool t3d_dw_row3_bwd_can(const DwShape& s);
T3D_DW_FWD(t3d_dw_row3_fwd);
T3D_DW_BWD(t3d_dw_row3_bwd);
// T3D_DW_PLANE7: dwconv5_plane7.hip
bool t3d_dw_plane7_can(const DwShape& s);
T3D_DW_FWD(t3d_dw_plane7_fwd);
T3D_DW_BWD(t3d_dw_plane7_bwd);
// T3D_DW_ROWK: dwconvk_stream.hip, dwconv5_bwd_stream.hip
bool t3d_dw_rowk_fwd_can(const DwShape& s);
bool t3d_dw_rowk_bwd_can(const DwShape& s);
T3D_DW_FWD(t3d_dw_rowk_fwd);
T3D_DW_BWD(t3d_dw_rowk_bwd);
// T3D_DW_LDS: dwconv_fwd.hip, dwconv_bwd.hip
bool t3d_dw_lds_can(const DwShape& s);
T3D_DW_FWD(t3d_dw_lds_fwd);
T3D_DW_BWD(t3d_dw_lds_bwd);
