// Pointwise (1x1) convolution entry points: validate, pick the kernel family ONCE by a pure function of the call's shape and
// options, settle the pending BatchNorm finalize, launch (pwconv_route.h).  Host code only.
#include "pwconv_route.h"

using namespace t3d_pw;

// include/t3d.h
extern "C" int t3d_bn_apply(int dtype, const void* y, const t3d_prologue* pro, const void* residual, void* z, int M, int C,
                            void* stream);

namespace {

int g_forced = T3D_PW_AUTO;   // t3d_pwconv_force_route

bool family_can(int route, const PwCall& c) {
  const bool wg = c.op == PW_WGRAD;
  switch (route) {
    case T3D_PW_DEEP: return deep_can(c);
    case T3D_PW_STREAM: return stream_can(c) || stream_f16_can(c);
    case T3D_PW_REG32: return wg ? reg32_wgrad_can(c) : reg32_can(c);
    case T3D_PW_LDS: return wg ? lds_wgrad_can(c) : lds_can(c);
    case T3D_PW_TR: return tr_can(c);
    default: return false;
  }
}
// automatic routing takes the first family of this list that can: the specialised kernels in front of the general one.  Every
// `can` names its dtypes and operations, so one list serves all calls: bf16 forward / data gradient DEEP, STREAM, LDS; fp16 STREAM;
// fp32 REG32, LDS; materialising forward STREAM (bf16) or REG32 (fp32); weight gradient TR (bf16) or REG32, LDS (fp32)
const int kOrder[] = {T3D_PW_DEEP, T3D_PW_STREAM, T3D_PW_REG32, T3D_PW_TR, T3D_PW_LDS};

// The finalize rule, here and nowhere else: the deep-contraction kernel, the bf16 streaming kernel and the bf16 weight-gradient
// kernel derive a pending BatchNorm finalize of the shared coefficients they read in their own prologue (t3d_take_fold in their
// launchers) -- for every other route, and for per-sample coefficients, the request becomes a launch of its own in front of the
// kernel.  (The y-free entries of pwconv_yfree.hip read no such coefficients in the streaming kernel.)
int settle(int route, const PwCall& c, const float* key, hipStream_t st) {
  const bool derives = route == T3D_PW_DEEP || route == T3D_PW_TR || (route == T3D_PW_STREAM && c.dtype == T3D_BF16);
  return derives && !c.per_sample ? T3D_OK : t3d_fold_fallback(key, st);
}

// forward, materialising forward, data gradient: settle and switch to the one launcher
int run(int route, const PwCall& c, GemmArgs& a, void* stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  a.wfrag = c.wfrag;
  if (const int rc = settle(route, c, a.p0, st)) return rc;
  switch (route) {
    case T3D_PW_DEEP: return deep_launch(c, a, st);
    case T3D_PW_STREAM: return c.dtype == T3D_BF16 ? stream_launch(c, a, st) : stream_launch_f16(c, a, st);
    case T3D_PW_REG32: return reg32_launch(c, a, st);
    default: return lds_launch(c, a, st);
  }
}

PwCall call(int op, int dtype, int M, int HW, int Kin, int Nout) {
  PwCall c{};
  c.op = op; c.dtype = dtype & ~T3D_W_FRAG; c.wfrag = (dtype & T3D_W_FRAG) != 0;
  c.M = M; c.HW = HW; c.Kin = Kin; c.Nout = Nout;
  return c;
}

}  // namespace

int t3d_pw::t3d_pw_route(const PwCall& c) {
  const bool sizes = c.M > 0 && c.HW > 0 && c.Kin > 0 && c.Nout > 0 && !(c.Kin % 8) && !(c.Nout % 8);
  if (c.op == PW_FWD_STATS) {   // the BatchNorm sums of a conv whose output is never stored (t3d_expdw_fwd recomputes it in LDS)
    const bool stream = g_forced == T3D_PW_AUTO || g_forced == T3D_PW_STREAM;
    return sizes && stream && stream_can(c) ? T3D_PW_STREAM : T3D_ERR_UNSUPPORTED;
  }
  if (!sizes || c.dtype < T3D_F32 || c.dtype > T3D_F16) return T3D_ERR_ARG;
  if (c.wfrag && c.dtype == T3D_F32) return T3D_ERR_ARG;                              // fragment-order weights are 16-bit
  if (c.op == PW_MAT && c.gated) return T3D_ERR_ARG;                                  // a block output is never gated
  if (c.op == PW_WGRAD && (c.wfrag || c.dtype == T3D_F16)) return T3D_ERR_ARG;        // (fp16 is inference forward only)
  // the materialising forward without a kernel of its own is the two launches it fuses -- which read row-major weights
  const int none = c.op != PW_MAT ? T3D_ERR_UNSUPPORTED : !c.wfrag ? T3D_PW_PAIR : c.dtype == T3D_BF16 ? T3D_ERR_UNSUPPORTED : T3D_ERR_ARG;
  if (g_forced != T3D_PW_AUTO) return family_can(g_forced, c) ? g_forced : (none == T3D_PW_PAIR ? none : T3D_ERR_UNSUPPORTED);
  for (const int r : kOrder)
    if (family_can(r, c)) return r;
  return none;
}

extern "C" int t3d_pwconv_route(int op, int dtype, int gated, int per_sample, int ps_stats, int e_se, int bias, int stats,
                                int alpha_gamma, int act, int residual, int M, int HW, int K, int N) {
  if (op < PW_FWD || op > PW_WGRAD) return T3D_ERR_ARG;
  const bool bwd = op == PW_DGRAD || op == PW_WGRAD;   // the contraction of the data gradient runs over the forward OUTPUT channels
  PwCall c = call(op, dtype, M, HW, bwd ? N : K, bwd ? K : N);
  // (a flag the operation's entry point has no argument for is ignored)
  const bool fwd = !bwd, dg = op == PW_DGRAD;
  c.gated = gated && !dg; c.per_sample = per_sample && bwd; c.ps_stats = ps_stats && dg; c.e_se = e_se && dg;
  c.bias = bias && (op == PW_FWD || op == PW_FWD_STATS); c.stats = stats && op != PW_WGRAD; c.alpha_gamma = alpha_gamma && bwd;
  c.act = fwd ? act : T3D_ACT_NONE; c.residual = residual && op == PW_MAT;
  return t3d_pw_route(c);
}

extern "C" int t3d_pwconv_force_route(int route) {
  if (route != T3D_PW_AUTO && (route < 0 || route > T3D_PW_TR)) return T3D_ERR_ARG;
  g_forced = route;
  return T3D_OK;
}

extern "C" int t3d_pwconv_fwd(int dtype, const void* x, const t3d_prologue* pro, const void* w, const float* bias,
                              void* y, double* stats, int M, int HW, int K, int N, void* stream) {
  if (!x || !w || (!y && !stats)) return T3D_ERR_ARG;
  PwCall c = call(y ? PW_FWD : PW_FWD_STATS, dtype, M, HW, K, N);
  c.gated = pro && pro->se; c.act = pro ? pro->act : T3D_ACT_NONE; c.bias = bias != nullptr; c.stats = stats != nullptr;
  const int route = t3d_pw_route(c);
  if (route < 0) return route;
  GemmArgs a{};
  a.a0 = x;
  if (pro) { a.p0 = pro->scale; a.p1 = pro->shift; a.p2 = pro->se; a.act = pro->act; a.se_after = pro->se_after_act; }
  a.w = w; a.bias = bias; a.out = y; a.stats = stats;
  a.M = M; a.HW = HW; a.Kin = K; a.Nout = N;
  return run(route, c, a, stream);
}

extern "C" int t3d_pwconv_fwd_mat(int dtype, const void* y_in, const t3d_prologue* pro_in, const void* residual, void* z_out,
                                  const void* w, void* y, double* stats, int M, int HW, int K, int N, void* stream) {
  if (!y_in || !pro_in || !z_out || !w || !y) return T3D_ERR_ARG;
  PwCall c = call(PW_MAT, dtype, M, HW, K, N);
  c.gated = pro_in->se != nullptr; c.act = pro_in->act; c.residual = residual != nullptr; c.stats = stats != nullptr;
  const int route = t3d_pw_route(c);
  if (route < 0) return route;
  if (route == T3D_PW_PAIR) {
    // t3d_bn_apply derives a pending finalize itself.  (Chosen automatically in fp32 the finalize stays a launch of its own, as
    // it has been since the register kernel's launcher was asked first; T3D_PW_LDS forced is the older order without it.)
    if (c.dtype == T3D_F32 && g_forced == T3D_PW_AUTO)
      if (const int rc = t3d_fold_fallback(pro_in->scale, reinterpret_cast<hipStream_t>(stream))) return rc;
    if (const int rc = t3d_bn_apply(c.dtype, y_in, pro_in, residual, z_out, M, K, stream)) return rc;
    return t3d_pwconv_fwd(c.dtype, z_out, nullptr, w, nullptr, y, stats, M, HW, K, N, stream);
  }
  GemmArgs a{};
  a.a0 = y_in;
  a.p0 = pro_in->scale; a.p1 = pro_in->shift; a.act = pro_in->act;
  a.z_res = residual; a.z_out = z_out;
  a.w = w; a.out = y; a.stats = stats;
  a.M = M; a.HW = HW; a.Kin = K; a.Nout = N;
  return run(route, c, a, stream);
}

extern "C" int t3d_pwconv_dgrad(int dtype, const void* dz, const void* y, const t3d_bnbwd* bb, const void* wt,
                                const void* x_raw, const t3d_prologue* pro_in, const void* residual, void* dx,
                                double* stats, float* ps_stats, int M, int HW, int K, int N, void* stream) {
  if (!dz || !y || !bb || !wt || !dx || !bb->beta) return T3D_ERR_ARG;
  PwCall c = call(PW_DGRAD, dtype, M, HW, N, K);  // contraction runs over the forward OUTPUT channels
  c.per_sample = bb->per_sample != 0; c.alpha_gamma = bb->alpha && bb->gamma; c.e_se = x_raw && pro_in && pro_in->se;
  c.stats = stats != nullptr; c.ps_stats = ps_stats != nullptr;
  const int route = t3d_pw_route(c);
  if (route < 0) return route;
  GemmArgs a{};
  a.dgrad = 1;
  a.a0 = dz; a.a1 = y;
  a.p0 = bb->alpha; a.p1 = bb->beta; a.p2 = bb->gamma; a.per_sample = bb->per_sample;
  a.w = wt;
  if (x_raw) {
    a.e_y = x_raw;
    if (pro_in) {
      a.e_scale = pro_in->scale; a.e_shift = pro_in->shift; a.e_se = pro_in->se;
      a.e_act = pro_in->act; a.e_se_after = pro_in->se_after_act;
    }
  }
  a.e_res = residual; a.out = dx; a.stats = stats; a.ps_stats = ps_stats;
  a.M = M; a.HW = HW; a.Kin = N; a.Nout = K;
  return run(route, c, a, stream);
}

extern "C" int t3d_pwconv_wgrad(int dtype, const void* dz, const void* y, const t3d_bnbwd* bb, const void* x,
                                const t3d_prologue* pro, float* dw, int M, int HW, int K, int N, void* stream) {
  if (!dz || !y || !bb || !x || !dw) return T3D_ERR_ARG;
  PwCall c = call(PW_WGRAD, dtype, M, HW, N, K);
  c.gated = pro && pro->se; c.per_sample = bb->per_sample != 0; c.alpha_gamma = bb->alpha && bb->gamma;
  const int route = t3d_pw_route(c);
  if (route < 0) return route;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (const int rc = settle(route, c, bb->alpha, st)) return rc;
  switch (route) {
    case T3D_PW_TR: return tr_launch(c, dz, y, bb, x, pro, dw, st);
    case T3D_PW_REG32:
      return reg32_wgrad_launch(c, reinterpret_cast<const float*>(dz), reinterpret_cast<const float*>(y), bb,
                                reinterpret_cast<const float*>(x), pro, dw, st);
    default: return lds_wgrad_launch(c, dz, y, bb, x, pro, dw, st);
  }
}
