// Shared between the pointwise-conv GEMM kernels (pwconv.hip: LDS-staged, fp32 + bf16; pwconv_stream.hip: barrier-free
// streaming kernel, bf16 / fp16; pwconv_deep.hip; pwconv_f32_reg.hip).  Their launchers: pwconv_route.h.
#pragma once
#include "common.h"

namespace t3d_pw {

struct GemmArgs {
  const void* a0;   // FWD: x (raw or finished); DGRAD: dz
  const void* a1;   // DGRAD: y (raw output of the differentiated conv), else null
  const float *p0, *p1, *p2;  // FWD: scale, shift, se[B][K]; DGRAD: alpha, beta, gamma
  int act, se_after, per_sample, dgrad;
  const void* w;     // [Nout][Kin] storage dtype
  const float* bias; // [Nout] or null
  const void* e_y;   // DGRAD epilogue: raw input tensor of the forward conv [M][Nout]
  const float *e_scale, *e_shift, *e_se;
  int e_act, e_se_after;
  const void* e_res;  // residual gradient to add [M][Nout]
  void* out;
  double* stats;      // [2][Nout]
  float* ps_stats;    // [B][Nout][2] per-sample sums (SE case)
  int ps_wave;        // per-sample sums: a WAVE owns whole samples (small planes; set by the launcher), else the workgroup does
  int M, HW, Kin, Nout, mtiles;
  int kz;             // generic kernel: contraction split over blockIdx.z (fp32 plain products of few-pixel layers),
  float* part;        // ... partial tiles [kz][M][Nout] in the workspace
  // second activation segment (y-free data gradient, streaming kernel only): k-steps >= ks1 read a2 [M][Kin2];
  // `Kin` is then the padded total (ks1*32 + round_up(Kin2, 32)) and indexes the weight rows directly
  const void* a2;
  int Kin2, ks1;
  int row0;   // row stride (= channel count) of a0 / a1; equals Kin without a second segment
  const T3dFold* fold;   // BatchNorm finalize of the operand's coefficients derived in the prologue (streaming kernel only)
  // materialising forward (t3d_pwconv_fwd_mat, streaming kernel only): the operand is z = bf16(p0*a0 + p1 + z_res), i.e.
  // the finished block output that t3d_bn_apply would have written; the blocks of output chunk 0 also STORE it to z_out
  const void* z_res;
  void* z_out;
  int unused_[8];        // (where the implicit-3x3 gather's fields were: the kernels' argument layout, and so their code, stay as measured)
  int wfrag;             // `w` is the fragment-order copy (include/t3d.h: T3D_W_FRAG; streaming and deep-contraction kernels)
  T3dQuant quant;        // forward BatchNorm sums snapped onto a fixed grid (order-independent, common.h); q == 0: off
};

template <typename T> __device__ __forceinline__ void ldvec(const T* p, float* v);
template <> __device__ __forceinline__ void ldvec<float>(const float* p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
template <> __device__ __forceinline__ void ldvec<bf16_t>(const bf16_t* p, float* v) { Vec8<bf16_t>::load(p, v); }
template <typename T> __device__ __forceinline__ void stvec(T* p, const float* v);
template <> __device__ __forceinline__ void stvec<float>(float* p, const float* v) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
template <> __device__ __forceinline__ void stvec<bf16_t>(bf16_t* p, const float* v) { Vec8<bf16_t>::store(p, v); }


}  // namespace t3d_pw
