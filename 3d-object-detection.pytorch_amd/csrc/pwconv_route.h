// Pointwise (1x1) dispatch (pwconv_route.hip): t3d_pwconv_fwd / _fwd_mat / _dgrad / _wgrad pick ONE kernel family from the
// call's shape and options, settle a pending BatchNorm finalize and call that family's launcher -- a call that returns an error
// has launched nothing and consumed nothing.  Every family keeps a `can` predicate next to its launcher: the dtypes, options and
// shape limits its kernels are correct for (a forced route asks only this).  No family has shapes it can take and loses on, so
// the automatic choice is the first family of a fixed order that can.
// A launcher called with a call its `can` rejects returns T3D_ERR_ARG: it never answers "try the next one".
#pragma once
#include "pwconv_common.h"

namespace t3d_pw {

// FWD_STATS: t3d_pwconv_fwd with y == NULL; MAT: t3d_pwconv_fwd_mat
enum { PW_FWD = T3D_PW_OP_FWD, PW_FWD_STATS = T3D_PW_OP_FWD_STATS, PW_MAT = T3D_PW_OP_MAT, PW_DGRAD = T3D_PW_OP_DGRAD, PW_WGRAD = T3D_PW_OP_WGRAD };

struct PwCall {
  int op, dtype, wfrag;   // dtype without the T3D_W_FRAG flag
  int gated;         // squeeze-excite gate on the operand (FWD / WGRAD: pro->se)
  int per_sample;    // DGRAD / WGRAD: per-sample BatchNorm-backward coefficients
  int ps_stats;      // DGRAD: per-sample sums wanted
  int e_se;          // DGRAD: gate in the epilogue (pro_in->se)
  int bias, stats;
  int alpha_gamma;   // DGRAD / WGRAD: bb->alpha and bb->gamma both present
  int act;           // FWD / MAT: the operand's activation
  int residual;      // MAT: residual added to the materialised operand
  int M, HW, Kin, Nout;   // DGRAD: after the swap (the contraction runs over the forward OUTPUT channels)
  // the kernels' squeeze-excite / per-sample variants
  bool gen() const { return per_sample || ps_stats || e_se || (op != PW_DGRAD && gated); }
};

// route id (include/t3d.h: T3D_PW_*) or the negative error code of the entry point; makes no HIP call
int t3d_pw_route(const PwCall& c);

// T3D_PW_DEEP: pwconv_deep.hip (bf16, fragment-order weights)
bool deep_can(const PwCall& c);
int deep_launch(const PwCall& c, GemmArgs& a, hipStream_t st);
bool deep_shape(int Kin, int Nout);   // t3d_pwconv_wants_frag
// T3D_PW_STREAM: pwconv_stream.hip (bf16) and the same unit in fp16 storage, inference forward only (pwconv_stream_f16.hip)
bool stream_can(const PwCall& c);
int stream_launch(const PwCall& c, GemmArgs& a, hipStream_t st);
bool stream_f16_can(const PwCall& c);
int stream_launch_f16(const PwCall& c, GemmArgs& a, hipStream_t st);
// T3D_PW_REG32: pwconv_f32_reg.hip (forward, materialising forward, data gradient), pwconv_f32_wgrad.hip (weight gradient)
bool reg32_can(const PwCall& c);
int reg32_launch(const PwCall& c, GemmArgs& a, hipStream_t st);
bool reg32_wgrad_can(const PwCall& c);
int reg32_wgrad_launch(const PwCall& c, const float* dz, const float* y, const t3d_bnbwd* bb, const float* x, const t3d_prologue* pro,
                       float* dw, hipStream_t st);
// T3D_PW_LDS: pwconv.hip (forward, data gradient), pwconv_wgrad.hip (weight gradient, fp32)
bool lds_can(const PwCall& c);
int lds_launch(const PwCall& c, GemmArgs& a, hipStream_t st);
bool lds_wgrad_can(const PwCall& c);
int lds_wgrad_launch(const PwCall& c, const void* dz, const void* y, const t3d_bnbwd* bb, const void* x, const t3d_prologue* pro, float* dw,
                     hipStream_t st);
// T3D_PW_TR: pwconv_wgrad_tr.hip (weight gradient, bf16)
bool tr_can(const PwCall& c);
int tr_launch(const PwCall& c, const void* dz, const void* y, const t3d_bnbwd* bb, const void* x, const t3d_prologue* pro, float* dw,
              hipStream_t st);

}  // namespace t3d_pw
