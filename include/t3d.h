/* t3d.h -- C ABI of the MI355X-native 3D-box keypoint-regression hot path.
 *
 * The reference (sovrasov/3d-object-detection.pytorch) is 100 % Python and has no
 * FFI of its own: every device op on its hot path is an ATen call issued from
 *   torchdet3d/models/mobilenetv3.py:110-166   (conv / BN / activation / SE)
 *   torchdet3d/builders/model_builder.py:96-146 (pool, per-class heads, cls head)
 *   torchdet3d/losses/regression_losses.py, builders/loss_builder.py (losses)
 *   torchdet3d/evaluation/metrics.py:10-37     (ADD / SADD / accuracy)
 * Each entry point below names the reference call site it replaces.  The
 * library (libt3d_hip.so, hand-written HIP for gfx950) is what the reference's
 * Python would bind with ctypes.
 *
 * Conventions
 *   - plain pointers + sizes; all buffers are caller-allocated DEVICE memory,
 *     no ownership transfer, no hidden allocation or synchronisation;
 *   - every call only ENQUEUES on `stream` (a hipStream_t passed as void*);
 *   - activations are NHWC ("channels last"), storage dtype T3D_F32 or T3D_BF16,
 *     arithmetic always accumulates in fp32 (statistics in fp64);
 *   - channel counts are multiples of 8;
 *   - return 0 on success, a negative T3D_ERR_* otherwise.
 */
#ifndef T3D_H_
#define T3D_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { T3D_F32 = 0, T3D_BF16 = 1, T3D_F16 = 2 };    /* T3D_F16: INFERENCE forward only (round 4): t3d_stem_im2col[_u8], t3d_pwconv_fwd,
                                                         t3d_dwconv_fwd (k = 3), t3d_bn_apply, t3d_pool_fwd, t3d_pack_weight[s_batched] */
/* Weight layout flag of the 16-bit pointwise convolutions (round 4): `T3D_BF16 | T3D_W_FRAG` (or `T3D_F16 | ...`) as the dtype
 * argument of t3d_pwconv_fwd / t3d_pwconv_fwd_mat / t3d_pwconv_dgrad says that `w` / `wt` is the FRAGMENT-ORDER copy made by
 * t3d_pwconv_pack_frag (or by t3d_pack_weights_batched's `frag` / `frag_t` outputs) of the matrix the plain call takes.  The
 * deep-contraction kernel streams the fragments from L2 (csrc/pwconv_deep.hip; t3d_pwconv_wants_frag names its shapes), the
 * streaming kernel stages its weight chunk with one linear copy (csrc/pwconv_stream.hip); shapes neither of them takes return
 * T3D_ERR_UNSUPPORTED / T3D_ERR_ARG (the LDS-tiled fallback kernel reads the row-major matrix only). */
enum { T3D_W_FRAG = 0x100 };
enum { T3D_ACT_NONE = 0, T3D_ACT_RELU = 1, T3D_ACT_RELU6 = 2, T3D_ACT_HSWISH = 3 };
enum { T3D_OK = 0, T3D_ERR_ARG = -1, T3D_ERR_LAUNCH = -2, T3D_ERR_UNSUPPORTED = -3 };

/* How a consumer turns a stored RAW (pre-BatchNorm) tensor into its activated
 * input on load, so BN/activation/SE never cost a pass over HBM:
 *   u = scale[c]*x + shift[c]            (scale == NULL: u = x)
 *   se_after_act == 0:  a = act(u * se[b][c])      (expand layout, mobilenetv3.py:153-156)
 *   se_after_act == 1:  a = act(u) * se[b][c]      (no-expand layout, mobilenetv3.py:137-140)
 * se == NULL: no squeeze-excite factor. */
typedef struct {
  const float* scale;
  const float* shift;
  const float* se;
  int act;
  int se_after_act;
} t3d_prologue;

int t3d_version(void);

/* Depthwise k x k conv forward, k in {3,5}, stride in {1,2}, pad (k-1)/2.
 * Replaces nn.Conv2d(C,C,k,s,(k-1)//2,groups=C) + the following BatchNorm2d's
 * statistics pass (mobilenetv3.py:136-137,152-153).
 *   x [B,H,W,C] (dtype), w [C,k*k] fp32 (= the reference's [C,1,k,k]),
 *   y [B,Ho,Wo,C] raw output (dtype),
 *   stats  [2*C] fp64 or NULL: += sum(y), sum(y^2) per channel (must be zeroed by caller),
 *   gap_sum [B*C] fp32 or NULL: += sum over (Ho,Wo) of y per sample/channel (for SE). */
int t3d_dwconv_fwd(int dtype, const void* x, const t3d_prologue* pro, const float* w, void* y,
                   double* stats, float* gap_sum, int B, int H, int W, int C, int k, int stride,
                   void* stream);

/* BatchNorm training-mode statistics -> per-channel affine (mobilenetv3.py:113 etc.;
 * PyTorch defaults eps=1e-5, momentum=0.1, biased var to normalise, unbiased running var).
 *   stats [2*C] fp64 sums over `count` elements; scale = gamma*invstd, shift = beta - mean*scale.
 *   running_mean/var, num_batches_tracked may be NULL (not updated). */
int t3d_bn_finalize(const double* stats, int C, double count, const float* gamma, const float* beta,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float momentum, float eps, float* scale, float* shift, float* mean, float* invstd,
                    void* stream);

/* Eval-mode BatchNorm folded to the same per-channel affine from the running estimates. */
int t3d_bn_eval_affine(int C, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, void* stream);

/* ... for every BatchNorm of a model in ONE launch (an inference forward otherwise issues ~50 of them): desc = n rows
 * of int64 {gamma, beta, running_mean, running_var, scale, shift, C}, a DEVICE array. */
int t3d_bn_eval_affine_batched(const long long* desc, int n, float eps, void* stream);

/* BatchNorm backward as a per-channel affine of two tensors, applied by the consumer on load:
 *   dy = alpha*dz + beta*y + gamma      (dz: gradient at the BN output, y: raw BN input)
 * alpha/gamma are [C], or [B*C] when per_sample != 0 (a squeeze-excite gate sits between). */
typedef struct {
  const float* alpha;
  const float* beta;
  const float* gamma;
  int per_sample;
} t3d_bnbwd;

/* Pointwise (1x1) conv forward as an MFMA GEMM.  Replaces nn.Conv2d(K,N,1) / nn.Linear(K,N)
 * + the statistics pass of the BatchNorm that follows (mobilenetv3.py:120-121,142-143,148-149,
 * 158-159,192-193).
 *   x [M,K] rows = NHWC pixels (M = B*H*W, HW = H*W for per-sample SE indexing),
 *   w [N,K] in the storage dtype, bias [N] fp32 or NULL, y [M,N] raw output,
 *   stats [2*N] fp64 or NULL: += sum(y), sum(y^2) per output channel (caller zeroes). */
int t3d_pwconv_fwd(int dtype, const void* x, const t3d_prologue* pro, const void* w, const float* bias,
                   void* y, double* stats, int M, int HW, int K, int N, void* stream);

/* Fragment-order weights (no reference counterpart: a layout of the weights nn.Conv2d holds, mobilenetv3.py:142-159).
 * `w` [rows, cols] in a 16-bit storage type, row-major -> out[((T*KS + ks)*64 + lg*16 + lc)*8 + j] = w[row(T, lc)][32 ks + 8 lg + j],
 * row(T, lc) = 32 (T >> 1) + 8 (lc >> 2) + 4 (T & 1) + (lc & 3), T < 2 ceil(rows / 32), KS = ceil(cols / 32), zero past rows / cols:
 * the A operand of v_mfma_f32_16x16x32_{bf16,f16} for 16 output channels x 32 contraction elements is 1 KB contiguous (a wave
 * loads it with one fully coalesced instruction instead of 64 separate 16-byte requests), and the row permutation inside a
 * pair of tiles leaves every lane with 8 consecutive output channels of a 32-channel block.  t3d_pwconv_frag_bytes: size of
 * `out`.  t3d_pwconv_wants_frag(K, N): 1 where the layout pays -- the deep-contraction kernel's shapes (K >= 512 and an output
 * wider than the streaming kernel's LDS chunk) -- for a contraction over K into N output channels (forward: (K, N) of the
 * layer with `w`; data gradient: (N, K) with the copy of `wt`).  The flag itself is accepted for every shape the streaming
 * kernel takes as well (K, N multiples of 8, K <= 1920). */
int t3d_pwconv_frag_bytes(int rows, int cols);
int t3d_pwconv_wants_frag(int K, int N);
int t3d_pwconv_pack_frag(const void* w, void* out, int rows, int cols, void* stream);

/* Pointwise conv data gradient (autograd of the conv above + the surrounding BN/activation).
 *   dz [M,N], y [M,N]: gradient at / raw input of the BatchNorm after the conv, bb its backward affine;
 *   wt [K,N]: TRANSPOSED weight in the storage dtype;
 *   x_raw [M,K] + pro_in: raw tensor the forward conv read and how it was activated; if given the
 *     result is multiplied by act'(.) and sum(dx), sum(dx*x_raw) are accumulated into
 *     stats [2*K] fp64 (per channel) or ps_stats [B*K*2] fp32 (per sample, SE case);
 *   residual [M,K] or NULL is added (skip connection); dx [M,K]. */
int t3d_pwconv_dgrad(int dtype, const void* dz, const void* y, const t3d_bnbwd* bb, const void* wt,
                     const void* x_raw, const t3d_prologue* pro_in, const void* residual, void* dx,
                     double* stats, float* ps_stats, int M, int HW, int K, int N, void* stream);

/* Weight packing: fp32 master weight [rows,cols] -> storage dtype, optionally transposed to
 * [cols,rows] (the dgrad GEMM reads the transposed copy). */
int t3d_pack_weight(int dtype, const float* w, void* out, int rows, int cols, int transpose, void* stream);

/* Pointwise conv weight gradient: dw[N,K] (fp32, the reference's [N,K,1,1]) += dy^T * a, with
 * dy = bb(dz, y) and a = pro(x) recomputed on load; the caller zeroes dw once per step. */
int t3d_pwconv_wgrad(int dtype, const void* dz, const void* y, const t3d_bnbwd* bb, const void* x,
                     const t3d_prologue* pro, float* dw, int M, int HW, int K, int N, void* stream);

/* The pointwise entry points (t3d_pwconv_fwd / _fwd_mat / _dgrad / _wgrad) pick ONE kernel family per call, by a pure function of
 * the call's dtype, options and sizes (csrc/pwconv_route.hip), ahead of every side effect.  Route ids:
 *   T3D_PW_DEEP    deep contractions with fragment-order weights (csrc/pwconv_deep.hip; bf16, t3d_pwconv_wants_frag's shapes)
 *   T3D_PW_STREAM  streaming kernel (csrc/pwconv_stream.hip: bf16, K <= 1920; fp16: inference forward)
 *   T3D_PW_REG32   fp32 register-operand kernels (csrc/pwconv_f32_reg.hip; weight gradient: pwconv_f32_wgrad.hip), M >= 1024
 *   T3D_PW_LDS     LDS-tiled kernels (csrc/pwconv.hip, pwconv_wgrad.hip): fp32 and bf16, row-major weights
 *   T3D_PW_TR      bf16 weight gradient (csrc/pwconv_wgrad_tr.hip)
 *   T3D_PW_PAIR    not a kernel: t3d_pwconv_fwd_mat runs the two calls it fuses, t3d_bn_apply + t3d_pwconv_fwd
 * t3d_pwconv_route RETURNS the route id of such a call, or the negative T3D_ERR_* the entry point would return; it makes no
 * device call.  op: T3D_PW_OP_* (FWD_STATS: t3d_pwconv_fwd with y == NULL); dtype may carry T3D_W_FRAG; the flags say what the call
 * passes: gated = pro->se, per_sample = bb->per_sample, ps_stats / bias / stats / residual = that pointer non-NULL, e_se = x_raw and
 * pro_in->se, alpha_gamma = bb->alpha and bb->gamma non-NULL, act = the operand's activation; M, HW, K, N as the entry point takes
 * them.  The fp32 weight gradient also reads the size of the workspace (t3d_set_workspace).
 * t3d_pwconv_force_route (tests and timing tools only; process-wide, T3D_PW_AUTO clears it): while a family is forced, calls it
 * can take go to it and every other call returns T3D_ERR_UNSUPPORTED, launching nothing -- except that t3d_pwconv_fwd_mat with
 * row-major weights answers T3D_PW_PAIR, whose convolution is routed under the same force. */
enum { T3D_PW_AUTO = -1, T3D_PW_DEEP = 0, T3D_PW_STREAM = 1, T3D_PW_REG32 = 2, T3D_PW_LDS = 3, T3D_PW_TR = 4, T3D_PW_PAIR = 5 };
enum { T3D_PW_OP_FWD = 0, T3D_PW_OP_FWD_STATS = 1, T3D_PW_OP_MAT = 2, T3D_PW_OP_DGRAD = 3, T3D_PW_OP_WGRAD = 4 };
int t3d_pwconv_route(int op, int dtype, int gated, int per_sample, int ps_stats, int e_se, int bias, int stats, int alpha_gamma,
                     int act, int residual, int M, int HW, int K, int N);
int t3d_pwconv_force_route(int route);

/* "y-free" backward of a pointwise conv whose input x [M,K] is a finished (materialised) bf16 tensor -- the expand
 * layer nn.Conv2d(K, N, 1) + nn.BatchNorm2d(N) of an inverted-residual block (models/mobilenetv3.py:148-149).
 * Because y = x W^T, the BatchNorm-backward affine dy = alpha*dz + beta*y + gamma never needs the wide tensor y:
 *   dx = [dz | x] Wcat^T + c,           Wcat = [alpha.W | W^T diag(beta) W] (bf16 [K][rup32(N)+rup32(K)]), c = gamma^T W
 *   dW += alpha.(dz^T x) + beta.(W (x^T x)) + gamma (1^T x)
 * Same sums as t3d_pwconv_dgrad / t3d_pwconv_wgrad, reassociated; bf16 storage only, per-channel bb only.
 *   _prep: wt [K,N] bf16 (the TRANSPOSED packed weights, as the data gradient reads them) -> wcat, cvec [K] fp32;
 *   _dgrad_yfree: x_raw / pro_in / residual / stats exactly as in t3d_pwconv_dgrad (x itself is the finished tensor the
 *     conv read; x_raw the raw tensor of its producer, for that producer's BatchNorm-backward sums); dx [M,K] bf16;
 *   _wgrad_yfree: needs t3d_set_workspace (returns T3D_ERR_UNSUPPORTED without it); dw [N,K] fp32 is accumulated. */
int t3d_pwconv_yfree_prep(const void* wt, const t3d_bnbwd* bb, void* wcat, float* cvec, int K, int N, void* stream);
int t3d_pwconv_dgrad_yfree(const void* dz, const void* x, const void* wcat, const float* cvec, const void* x_raw,
                           const t3d_prologue* pro_in, const void* residual, void* dx, double* stats, int M, int HW,
                           int K, int N, void* stream);
int t3d_pwconv_wgrad_yfree(const void* dz, const void* x, const t3d_bnbwd* bb, const void* w, float* dw, int M, int HW,
                           int K, int N, void* stream);

/* The same y-free backward with ONE pass over the wide gradient tensor (round 4): the pair above reads dz [M,N] twice, at the
 * same time from two streams; t3d_pwconv_bwd_yfree forms dx AND the partial tiles of [dz | x | 1]^T x from the same staged rows.
 *   _prep2: as _prep, plus wd -- the weights in the staged rows' column order, [16*ceil(K/16)][64*ceil((N+K+8)/64)] bf16,
 *     cleared once by the caller (only the non-zero entries are written each step);
 *   _bwd_yfree_scratch: RETURNS the bytes of `scratch` a launch of this shape needs (a query, not a status code; 0: shape not
 *     supported -- K <= 32, 64 < N + K + 8 <= 256);
 *   _bwd_yfree (the caller's main stream): dx [M,K] bf16 = [dz | x | 1] wd^T (+ residual), stats += sum(dx), sum(dx*x_raw)
 *     (x_raw / pro_in as in t3d_pwconv_dgrad; only a linear producer -- no activation -- is supported), partial tiles -> scratch;
 *   _wgrad_yfree_finish (any stream ordered behind it): dw [N,K] += the combined weight gradient, from `scratch`.
 * Replaces the autograd of nn.Conv2d(K, N, 1) + nn.BatchNorm2d(N) (models/mobilenetv3.py:148-149), as the pair does. */
int t3d_pwconv_yfree_prep2(const void* wt, const t3d_bnbwd* bb, void* wcat, float* cvec, void* wd, int K, int N, void* stream);
/* _bwd_yfree_w (round 5): t3d_pwconv_bwd_yfree with the weight rows `wd` built in the launch's own prologue from wt [K,N] (the
 * transposed bf16 weights) and the BatchNorm-backward coefficients `bb` (or the pending finalize request for them): the same
 * numbers bit for bit, without the t3d_pwconv_yfree_prep2 launch in front of it on the critical stream. */
int t3d_pwconv_bwd_yfree_w(const void* dz, const void* x, const void* wt, const t3d_bnbwd* bb, const void* x_raw,
                           const t3d_prologue* pro_in, const void* residual, void* dx, double* stats, void* scratch,
                           long long scratch_bytes, int M, int HW, int K, int N, void* stream);
int t3d_pwconv_bwd_yfree_scratch(int M, int K, int N);
int t3d_pwconv_bwd_yfree(const void* dz, const void* x, const void* wd, const void* x_raw, const t3d_prologue* pro_in,
                         const void* residual, void* dx, double* stats, void* scratch, long long scratch_bytes, int M, int HW,
                         int K, int N, void* stream);
int t3d_pwconv_wgrad_yfree_finish(void* scratch, const t3d_bnbwd* bb, const void* w, float* dw, int M, int K, int N, void* stream);

/* Depthwise conv backward: data gradient and weight gradient in one pass.
 *   dz, y [B,Ho,Wo,C]: gradient at / raw input of the BatchNorm after the conv; bb its backward affine;
 *   w [C,k*k] fp32; x [B,H,W,C] + pro: tensor the forward conv read and how it was activated (no SE);
 *   residual [B,H,W,C] or NULL is added; dx [B,H,W,C];
 *   stats [2*C] fp64 or NULL: += sum(dx), sum(dx*x); dw [C,k*k] fp32 or NULL: += weight gradient. */
int t3d_dwconv_bwd(int dtype, const void* dz, const void* y, const t3d_bnbwd* bb, const float* w,
                   const void* x, const t3d_prologue* pro, const void* residual, void* dx, double* stats,
                   float* dw, int B, int H, int W, int C, int k, int stride, void* stream);

/* Which kernel family a depthwise call takes.  Both entry points pick it once, ahead of any side effect, by a pure function
 * of the call's shape: a call that returns an error has launched nothing and has left a pending t3d_fold_request pending.
 *   T3D_DW_TILE    register tiles (csrc/dwconv_tile.hip): 5x5 on 8x8 ... 64x64 planes (28x28 at stride 2), pooled 3x3 up to 14x14
 *   T3D_DW_ROW3    3x3 row walk (csrc/dwconv3_stream.hip, dwconv3_bwd_stream.hip; backward: tensors below 2 GB)
 *   T3D_DW_PLANE7  5x5 stride 1 on 7x7 planes (csrc/dwconv5_plane7.hip)
 *   T3D_DW_ROWK    k x k row walk (csrc/dwconvk_stream.hip; backward 5x5: dwconv5_bwd_stream.hip)
 *   T3D_DW_LDS     LDS tiles (csrc/dwconv_fwd.hip, dwconv_bwd.hip): the only family with a gated input
 * t3d_dwconv_route RETURNS the route id of such a call, or the negative T3D_ERR_* the entry point would return; it makes no
 * device call.  gated_input: a squeeze-excite gate in the input prologue (pro->se); pooled: gap_sum != NULL (forward only).
 * t3d_dwconv_force_route (tests and timing tools only; process-wide, T3D_DW_AUTO clears it): while a route is forced, the
 * query and both entry points take that family wherever its kernels are correct -- measured faster or not -- and return
 * T3D_ERR_UNSUPPORTED, launching nothing, where they are not.
 * t3d_dwconv_plan returns what t3d_dwconv_route returns (a forced route included) and, for the two row-walk families, the
 * launch geometry their launcher takes (csrc/dwconv_walk.h: one planner, six specs): out[0..8] = rows per chunk, chunks,
 * slab mapping (0: flat), work items, grid.x, grid.y, weight-gradient slots needed, dynamic LDS bytes, template variant
 * (channels per thread; output columns per thread for the T3D_DW_ROWK forward).  Zeros for every other route or an error.
 * No device call. */
enum { T3D_DW_AUTO = -1, T3D_DW_TILE = 0, T3D_DW_ROW3 = 1, T3D_DW_PLANE7 = 2, T3D_DW_ROWK = 3, T3D_DW_LDS = 4 };
int t3d_dwconv_route(int backward, int dtype, int gated_input, int pooled, int B, int H, int W, int C, int k, int stride);
int t3d_dwconv_plan(int backward, int dtype, int gated_input, int pooled, int B, int H, int W, int C, int k, int stride,
                    int* out);
int t3d_dwconv_force_route(int route);

/* BatchNorm backward bookkeeping: from the reductions the gradient-producing kernel emitted,
 *   stats [2*C] fp64 = sum(dz), sum(dz*y)  over `count` elements (dz: gradient at the BN output,
 *   y: raw BN input), and the forward's mean / invstd, build the backward affine
 *   dy = alpha*dz + beta*y + gammac  and the parameter gradients (autograd of nn.BatchNorm2d in
 *   training mode, mobilenetv3.py:113 etc.):
 *     dbeta = sum(dz), dgamma = invstd*(sum(dz*y) - mean*sum(dz)),
 *     alpha = gamma*invstd, beta = -alpha*invstd*dgamma/count, gammac = -alpha*sum(dz)/count - beta*mean.
 *   dgamma / dbeta (may be NULL) are OVERWRITTEN. */
int t3d_bn_bwd_finalize(const double* stats, int C, double count, const float* gamma, const float* mean,
                        const float* invstd, float* alpha, float* beta, float* gammac, float* dgamma,
                        float* dbeta, void* stream);

/* Stem patch gather: crops x [B,3,H,W] fp32 NCHW (the reference's input contract,
 * dataloaders/objectron_main.py:51-96) -> col [B*Ho*Wo, 32] (dtype), the 3x3 / stride-2 / pad-1
 * patches of nn.Conv2d(3,C,3,2,1) (mobilenetv3.py:110-115) in (ci,ky,kx) order, columns 27..31 zero.
 * The stem conv itself then runs as t3d_pwconv_{fwd,wgrad} with K = 32. */
int t3d_stem_im2col(int dtype, const float* x, void* col, int B, int H, int W, void* stream);
/* The same gather from raw uint8 NHWC crops [B,H,W,3], normalised on the way: (u/255 - mean[c]) * inv_std[c]
 * (configs/default_config.py:9-10; padding taps are zeros of the NORMALISED image, as the reference's conv sees them).
 * The crops can then stay uint8 from the decoder to the GPU: 4x less PCIe / HBM than the fp32 tensor. */
int t3d_stem_im2col_u8(int dtype, const unsigned char* x, const float* mean, const float* inv_std, void* col, int B, int H,
                       int W, void* stream);

/* A whole inverted-residual block in inference mode (running statistics: every BatchNorm is a per-channel affine), bf16,
 * for the 14x14 / 7x7 stages: z = BN3(W2 * act2(BN2(dw3x3(act1(BN1(W1 * x)))))) [+ x], models/mobilenetv3.py:146-164 in
 * eval().  One workgroup per image keeps the expanded tensors in LDS (csrc/block_eval.hip); replaces
 * t3d_pwconv_fwd + t3d_dwconv_fwd + t3d_pwconv_fwd + t3d_bn_apply of that block with the same rounding points.
 * x [B,H,W,Cin] finished input, w1 [Ce,Cin], w2 [Cout,Ce] bf16, wdw [Ce,9] fp32, scale/shift fp32 per channel (eval affines),
 * z [B,H,W,Cout].  Stride 1, 3x3, no squeeze-excite; shapes outside the built set return T3D_ERR_UNSUPPORTED. */
int t3d_ir_block_eval(const void* x, const void* w1, const float* scale1, const float* shift1, int act1, const float* wdw,
                      const float* scale2, const float* shift2, int act2, const void* w2, const float* scale3,
                      const float* shift3, int residual, void* z, int B, int H, int W, int Cin, int Ce, int Cout, void* stream);

/* Two-stage inference, input side: crop every detection out of ONE full frame and resize it to the regressor's input
 * size, in one launch.  frame [H,W,3] uint8 (device), rects [n,4] int32 (x0,y0,x1,y1), device) -> out [n,oh,ow,3] uint8
 * NHWC.  Replaces the host loop `frame[y0:y1, x0:x1]` + `cv.resize(crop, (w, h))` per detection (utils/ie_wrappers.py:
 * 18-21,128-133,154-158; same crop as dataloaders/objectron_main.py:98-127): numpy slice semantics (bounds clamped to
 * the frame; an empty crop gives zeros) and cv::resize INTER_LINEAR's 8-bit arithmetic (half-pixel centres, replicated
 * border, 11-bit fixed-point weights) as restated in csrc/crop.hip -- bit-exact against oracle/crop_resize.py. */
int t3d_crop_resize_u8(const unsigned char* frame, const int* rects, unsigned char* out, int n, int H, int W, int oh, int ow,
                       void* stream);

/* The reference's training augmentations of a batch of crops, one launch (csrc/augment.hip; replaces the albumentations
 * pipeline of dataloaders/objectron_main.py:71-80 as builders/loader_builder.py:38-68 compiles configs/default_config.py:31-37):
 * per sample, in this order and with uint8 rounding after each step that yields an image,
 *   resize to (oh, ow)  cv::resize INTER_LINEAR on 8-bit data (t3d_crop_resize_u8's arithmetic),
 *   T3D_AUG_FLIP        mirror the columns (A.HorizontalFlip),
 *   T3D_AUG_LUT         lut[i] = (uint8) clip(float32(i) * alpha + beta255, 0, 255) (A.RandomBrightnessContrast, uint8),
 *   T3D_AUG_ROTATE      cv::warpAffine INTER_LINEAR, border 0, through the INVERSE map m (utils/transforms.py:50-89),
 *   T3D_AUG_SWAP_RB     RGB -> BGR (a pipeline without convert_color hands the model cv.imread's order).
 * src: the crops, each h rows of w*3 bytes, packed at `offset`; src_bytes bounds them (a record outside it, or with h or w
 * < 1, gives a zero image).  samples: [B] t3d_aug_sample in DEVICE memory.  out [B, oh, ow, 3] uint8, 4-byte aligned.
 * With no flag set the output equals t3d_crop_resize_u8 of the same crop, bit for bit. */
enum { T3D_AUG_FLIP = 1, T3D_AUG_LUT = 2, T3D_AUG_ROTATE = 4, T3D_AUG_SWAP_RB = 8 };
typedef struct {
  long long offset;      /* byte offset of the crop in src */
  int h, w;              /* crop size */
  int flags;             /* T3D_AUG_* */
  float alpha;           /* contrast (T3D_AUG_LUT) */
  float beta255;         /* brightness * 255, rounded to float32 once (T3D_AUG_LUT) */
  int reserved;
  double m[6];           /* T3D_AUG_ROTATE: output pixel -> resized-image coordinate, row-major 2x3 (fp64) */
} t3d_aug_sample;        /* 80 bytes */
int t3d_augment_crops_u8(const unsigned char* src, long long src_bytes, const void* samples, unsigned char* out, int B, int oh,
                         int ow, void* stream);

/* The same augmentations over crops that are already resized (csrc/augment.hip): t3d_augment_crops_u8 with its resize
 * stage replaced by a load.  Replaces the per-epoch `Objectron.__getitem__` + `A.Resize` of the reference
 * (dataloaders/objectron_main.py:51-96: every epoch decodes, crops and resizes every object again): resize(crop(frame)) is
 * the same image in every epoch, so the loader keeps it in device memory (dataloaders/gpu_loader.py, `cfg.data.cache`) and
 * an epoch is a gather from that arena with flip, LUT, rotation and channel swap applied on the way out.
 * arena: [oh, ow, 3] uint8 images, each at its record's byte `offset` (64-bit; any alignment); a record's h, w must equal
 * oh, ow.  A record with another size, a negative offset or one that reaches past arena_bytes gives a zero image.
 * samples: [B] t3d_aug_sample in DEVICE memory.  out [B, oh, ow, 3] uint8, 4-byte aligned.
 * When the arena images are t3d_augment_crops_u8's output with no flag set, the result equals t3d_augment_crops_u8 on the
 * original crops with the same flags, alpha, beta255 and m, bit for bit. */
int t3d_augment_resized_u8(const unsigned char* arena, long long arena_bytes, const void* samples, unsigned char* out, int B,
                           int oh, int ow, void* stream);

/* The augmentations of a pipeline that also names random_rescale (utils/transforms.py:20-47), hue_saturation_value or
 * color_jitter (builders/loader_builder.py:38-52), at most four launches (csrc/augment_chain.hip).  Per sample, with uint8
 * rounding after each step that yields an image:
 *   resize to (oh, ow), T3D_AUG_FLIP, T3D_AUG_LUT   as t3d_augment_crops_u8 (the base record `samples[i]`),
 *   the colour program `chains[i]`                  ops[0 .. n_ops) in order, each on the whole uint8 image:
 *     T3D_CHAIN_LUT         lut[i] = (uint8) clip(float32(i) * float32(p0) + float32(p1), 0, 255)   (T3D_AUG_LUT's arithmetic),
 *     T3D_CHAIN_HSV         RGB -> HSV (8-bit, H in 0..179), H = (uint8) mod(H + p0, 180), S = (uint8) clip(S + p1, 0, 255),
 *                           V = (uint8) clip(V + p2, 0, 255) in fp64 (numpy's mod: the sign of the divisor), HSV -> RGB,
 *     T3D_CHAIN_BRIGHTNESS  lut[i] = (uint8) clip(i * p0, 0, 255) in fp64,
 *     T3D_CHAIN_CONTRAST    lut[i] = (uint8) clip(i * p0 + mean * (1 - p0), 0, 255) in fp64; mean = (integer sum of the grey
 *                           image the op meets) / (oh * ow) in fp64.  At most one per program,
 *     T3D_CHAIN_SATURATION  rint(float32(x) * float32(p0) + float32(grey) * float32(1 - p0)), half to even, saturated,
 *     T3D_CHAIN_HUE         T3D_CHAIN_HSV with shifts (180 * p0, 0, 0),
 *     grey = (9798 R + 19235 G + 3735 B + 2^14) >> 15; the 8-bit HSV pair is restated at the top of csrc/augment_chain.hip,
 *   T3D_AUG_ROTATE        the first warp: cv::warpAffine INTER_LINEAR, border 0, through the inverse map m of the base record,
 *   T3D_CHAIN_WARP2       the second warp, through chains[i].m2, of the first warp's uint8 result (needs T3D_AUG_ROTATE),
 *   T3D_AUG_SWAP_RB       RGB -> BGR.
 * `stages` names the passes some record needs: T3D_STAGE_MEAN (a T3D_CHAIN_CONTRAST op: a reduction launch in front of the
 * colour launch), T3D_STAGE_WARP (T3D_AUG_ROTATE), T3D_STAGE_WARP2 (T3D_CHAIN_WARP2); a pass that is not named is not
 * launched.  A bad record gives a zero image and leaves the other samples alone: a base record t3d_augment_crops_u8
 * refuses, n_ops outside 0..8, an unknown op kind or flag, a second CONTRAST op, T3D_CHAIN_WARP2 without T3D_AUG_ROTATE,
 * or a record that needs a stage `stages` does not name.
 * samples: [B] t3d_aug_sample, chains: [B] t3d_aug_chain, both in DEVICE memory.  scratch: device memory, 8-byte aligned,
 * scratch_bytes >= 8 * B (the grey sums; zeroed by the call) + r * B * oh * ow * 3 rounded up to a multiple of 8, r = the
 * number of warp stages named (the uint8 images between the passes).  out [B, oh, ow, 3] uint8, 4-byte aligned.  B <= 65535.
 * With n_ops == 0 and no second warp the output equals t3d_augment_crops_u8 of the same base records, bit for bit. */
enum { T3D_CHAIN_LUT = 1, T3D_CHAIN_HSV = 2, T3D_CHAIN_BRIGHTNESS = 3, T3D_CHAIN_CONTRAST = 4, T3D_CHAIN_SATURATION = 5,
       T3D_CHAIN_HUE = 6 };
enum { T3D_CHAIN_WARP2 = 1 };
enum { T3D_STAGE_MEAN = 1, T3D_STAGE_WARP = 2, T3D_STAGE_WARP2 = 4 };
#define T3D_CHAIN_MAX_OPS 8
typedef struct {
  int n_ops;                         /* 0 .. T3D_CHAIN_MAX_OPS */
  int flags;                         /* T3D_CHAIN_WARP2 */
  int kind[T3D_CHAIN_MAX_OPS];       /* T3D_CHAIN_* of each op */
  double p[T3D_CHAIN_MAX_OPS][3];    /* its parameters (fp64) */
  double m2[6];                      /* T3D_CHAIN_WARP2: output pixel -> coordinate in the first warp's result, row-major 2x3 */
} t3d_aug_chain;                     /* 280 bytes */
int t3d_augment_chain_crops_u8(const unsigned char* src, long long src_bytes, const void* samples, const void* chains,
                               void* scratch, long long scratch_bytes, unsigned char* out, int B, int oh, int ow, int stages,
                               void* stream);

/* t3d_augment_chain_crops_u8 over an arena of crops that were resized once (the records t3d_augment_resized_u8 takes):
 * the same template over another source, so the two agree bit for bit as t3d_augment_resized_u8 / t3d_augment_crops_u8 do. */
int t3d_augment_chain_resized_u8(const unsigned char* arena, long long arena_bytes, const void* samples, const void* chains,
                                 void* scratch, long long scratch_bytes, unsigned char* out, int B, int oh, int ow, int stages,
                                 void* stream);

/* The detector's training pipeline on whole frames, one launch per batch, no scratch, no atomics (csrc/detect_augment.hip;
 * replaces the CPU workers' per-pixel work of configs/detection/mnv2_ssd_300_2_heads.py:71-101).  The semantics are those of
 * the PUBLISHED mmdet 2.x transforms; the fork that ran the config is external, so parity with it is UNPINNED: this comment
 * and tests/detect_augment_ref.py are the definition.  Per sample, in the config's order:
 *   PhotoMetricDistortion   on float32 RGB, unclipped between steps, each operation rounded to float32 on its own:
 *     T3D_DET_BRIGHTNESS    x + delta
 *     T3D_DET_CONTRAST      x * alpha, in front of the HSV block, or behind it with T3D_DET_CONTRAST_LAST
 *     T3D_DET_HSV           the RGB -> HSV -> RGB round trip (mmdet always makes it), OpenCV's float32 form:
 *                             v = max, diff = v - min, s = diff / (|v| + FLT_EPSILON), d = 60 / (diff + FLT_EPSILON),
 *                             h = v == r ? (g - b) d : v == g ? (b - r) d + 120 : (r - g) d + 240, h += 360 if h < 0;
 *                           T3D_DET_SATURATION  s * sat;   T3D_DET_HUE  h + hue, then h -= 360 if h > 360, h += 360 if h < 0;
 *                             hf = h * (6 / 360) (+ 6 once if < 0, - 6 once if >= 6), sector = floor(hf) (outside 0..5: sector 0,
 *                             f = 0), f = hf - sector, tab = {v, v(1 - s), v(1 - s f), v(1 - s(1 - f))}, OpenCV's sector table
 *     perm                  out channel c = channel perm[c]
 *   quarter turns           np.rot90(frame, turns), turns in {0, 1, 3}
 *   Expand                  the turned frame pasted at (left, top) into a canvas of fill 0 (the fill is not distorted)
 *   MinIoURandomCrop        the canvas rectangle [cx0, cx1) x [cy0, cy1)
 *   Resize                  to (oh, ow), bilinear in float32: the coordinate rule of cv::resize (csrc/resize_linear.h: half-pixel
 *                           centres, fraction zeroed at the column borders, rows clipped) with weights 1 - f and f; horizontal
 *                           pass d = a * (1 - fx) + b * fx, then vertical, every product and sum rounded on its own
 *   T3D_DET_FLIP            mirror the columns
 *   output                  rint (half to even), saturated to uint8, NHWC RGB -- the stem's uint8 contract.  DEVIATION: mmdet
 *                           hands the network the unclipped float32 / 255; here the result is rounded and saturated once.
 * The kernel fuses the geometry into one gather per output pixel: the four taps of the resize are translated to canvas
 * coordinates; a tap outside the pasted frame is 0, a tap inside is turned back to a source pixel, loaded as uint8 and
 * distorted before it is interpolated.  Whatever lies outside the pasted frame is fill, so the crop is not checked against
 * the canvas (whose size the kernel does not need).
 * src: the frames, each h rows of w*3 bytes, packed at `offset`; src_bytes bounds them.  samples: [B] t3d_det_sample in DEVICE
 * memory.  out [B, oh, ow, 3] uint8, ANY alignment (dword stores where the address allows).  B <= 65535.
 * A bad record gives a zero image and leaves the other images alone: h or w < 1, offset < 0 or offset + h*w*3 > src_bytes,
 * turns not in {0, 1, 3}, perm not a permutation of (0, 1, 2), an unknown flag, an empty crop (cx1 <= cx0 or cy1 <= cy0) or
 * one wider or higher than 2^24.  No record makes the kernel read outside [src, src + src_bytes) or write outside its image. */
enum { T3D_DET_FLIP = 1, T3D_DET_BRIGHTNESS = 2, T3D_DET_CONTRAST = 4, T3D_DET_CONTRAST_LAST = 8, T3D_DET_HSV = 16,
       T3D_DET_SATURATION = 32, T3D_DET_HUE = 64 };
typedef struct {
  long long offset;      /* byte offset of the frame in src */
  int h, w;              /* frame size */
  int turns;             /* quarter turns in np.rot90's sense: 0, 1 or 3 */
  int left, top;         /* where the turned frame is pasted in the canvas */
  int cx0, cy0, cx1, cy1;/* the crop in canvas coordinates, half open */
  int flags;             /* T3D_DET_* */
  float delta;           /* T3D_DET_BRIGHTNESS */
  float alpha;           /* T3D_DET_CONTRAST */
  float sat;             /* T3D_DET_SATURATION */
  float hue;             /* T3D_DET_HUE, degrees */
  int perm[3];           /* output channel c is distorted channel perm[c] */
  int reserved;
} t3d_det_sample;        /* 80 bytes */
int t3d_detect_augment_u8(const unsigned char* src, long long src_bytes, const void* records, unsigned char* out, int B, int oh,
                          int ow, void* stream);

/* t3d_detect_draw: the records t3d_detect_augment_u8 takes and the batch's ground truth, made ON THE DEVICE in one launch from
 * tables that live there (csrc/detect_draw.hip, csrc/detect_draw.h; torchdet3d/dataloaders/detection_arena.py).  It does what
 * DetectionAugmentPipeline.draw, .boxes and .records do on the host (torchdet3d/dataloaders/detection.py) and gives THEIR
 * RESULTS BIT FOR BIT from the same key; tests/test_detect_draw_host.py holds t3d_detect_draw_host to them.
 * t3d_detect_draw_host is the same arithmetic on the CPU: the same arguments, every pointer a HOST pointer, `stream` ignored;
 * HOST ONLY, no HIP call, never initialises the GPU.
 *   cfg [n_cfg = 34] doubles, HOST memory (both entry points): the compiled pipeline, by position
 *        0  PhotoMetricDistortion present (0 / 1)     1  brightness_delta     2, 3  contrast_range     4, 5  saturation_range
 *        6  hue_delta     7  probability of the quarter turn     8, 9  Expand's ratio_range (1, 1 without)     10  Expand's prob
 *        11  MinIoURandomCrop present     12  min_crop_size     13  1: `iou.min() < mode` compares in float32 (numpy >= 2: a
 *        Python float is weak), 0: in float64     14  number of crop modes, <= 16     15 .. 30  the modes (1 = the whole canvas;
 *        with a crop one of them must be 1)     31  flip_ratio     32  oh     33  ow
 *   key [n_key <= 16] uint32, HOST memory: the words numpy's SeedSequence makes of (seed, epoch, rank, batch) -- each integer
 *        as its 32-bit words, low word first, at least one
 *   frames int64 [B, 4]    per sample (byte offset of the decoded frame, h, w, dataset index)
 *   boxes float32 [n_boxes, 4], labels int32 [n_boxes], box_start int64 [n_images + 1]: image j owns the rows
 *        box_start[j] .. box_start[j + 1] - 1
 *   records [B] t3d_det_sample (byte-identical to records()); gt_boxes float32 [B, G, 4] in output pixels; gt_labels int32 [B, G];
 *   gt_counts int32 [B]; every row past a count is zero.  diag int32 [B, 2]: the index of the crop mode that returned (-1
 *   without a crop) and the number of uniforms the crop search drew (saturated at 2^31 - 1).
 * Random numbers: numpy's.  SeedSequence (pool of 4 words, hash-mix constants 0x43b0d7e5 / 0x931e8875 / 0x8b51f9dd / 0x58f38ded /
 * 0xca01f9dd / 0x4973f715, generate_state of eight words) seeds PCG64 (state = state * 0x2360ED051FC65DA44385DF649FCCF645 + inc
 * in 128 bits, XSL-RR output); random() = (next64 >> 11) * 2^-53.  The batch's generator is default_rng(key).random((B, 18)):
 * sample i owns outputs 18 i .. 18 i + 17 (columns: DetectionAugmentPipeline.draw) and reaches them by the LCG's jump-ahead.
 * The crop search of sample i draws from its own generator keyed (*key, 0x0A7E11F2, 0x5D3C, i).
 * Arithmetic: float64 where the host computes with Python floats (the photometric parameters before their cast, Expand's
 * ratio, canvas and paste position, the crop's new_w / new_h, aspect test, left / top and their truncation, the ow / cw scale
 * before its cast), float32 where it computes on float32 arrays (the turn, the shift, IoU with max(union, 1e-6) and its
 * division, centres, clip, scale, flip); every operation rounded on its own, no fused multiply-add.  Loops: 50 tries a mode, a
 * fresh mode after 50 failures, without bound; mode 1 returns the whole canvas.
 * One sample a wave, lane 0 walks: the launch lasts as long as its longest search.
 * T3D_ERR_ARG, nothing launched: a NULL pointer, n_cfg != 34, n_key < 1 or > 16, B < 0 or > 65535, G < 1 or > 64, negative
 * table sizes, oh or ow < 1, a ratio_range outside 1 <= lo <= hi <= 64, with a crop: no mode or more than 16, min_crop_size
 * outside (0, 1], no mode equal to 1.  B == 0 returns T3D_OK.
 * A bad sample gets a ZERO record (a zero image, by t3d_detect_augment_u8's rule), count 0 and diag (-1, 0), and the others are
 * left alone: h or w < 1 or > 2^24, offset < 0, a dataset index outside [0, n_images), a box range outside [0, n_boxes] or
 * longer than G.  Nothing is read outside the tables or written outside the sample's own rows. */
int t3d_detect_draw(const double* cfg, int n_cfg, const unsigned int* key, int n_key, const long long* frames, int B,
                    const float* boxes, const int* labels, const long long* box_start, long long n_images, long long n_boxes, int G,
                    void* records, float* gt_boxes, int* gt_labels, int* gt_counts, int* diag, void* stream);
int t3d_detect_draw_host(const double* cfg, int n_cfg, const unsigned int* key, int n_key, const long long* frames, int B,
                         const float* boxes, const int* labels, const long long* box_start, long long n_images, long long n_boxes,
                         int G, void* records, float* gt_boxes, int* gt_labels, int* gt_counts, int* diag, void* stream);

/* Baseline JPEG frames decoded on the device from a per-file index (csrc/jpeg_index.h, csrc/jpeg.hip; replaces the workers'
 * Pillow decode in front of t3d_detect_augment_u8).  Huffman decoding is serial inside a scan and Objectron frames carry no
 * restart markers, so ONCE PER FILE the host walks the scan (t3d_jpeg_index) and records where every seg_mcus-th MCU starts;
 * every epoch the device decodes all segments of all frames of a batch in parallel (t3d_jpeg_decode_u8).
 *
 * Supported: baseline sequential (SOF0), 8 bit, ONE interleaved scan, no restart interval, one component (gray) or three with
 * sampling 1x1/1x1/1x1 (4:4:4) or 2x2/1x1/1x1 (4:2:0), YCbCr.  Anything else is T3D_ERR_UNSUPPORTED with info->reason set;
 * malformed input (bad lengths, missing tables, a code that does not exist, a run past coefficient 63, a marker or the end of
 * the data inside the scan, no EOI behind it) is T3D_ERR_ARG.  The indexer decodes the whole scan: a file it accepts is
 * decodable to its last MCU, and the device is only ever given such files.
 *
 * DEFINITION (libjpeg / libjpeg-turbo's default path: JDCT_ISLOW, fancy upsampling; restated in numpy by tests/jpeg_ref.py;
 * bit-exact against Pillow on libjpeg-turbo for streams whose dequantised coefficients fit int16 -- every encoder-made file;
 * outside that libjpeg's own SIMD and C paths differ and the int32 arithmetic below is the definition):
 *   entropy    baseline Huffman.  DC: category t, t more bits v, diff = v < 2^(t-1) ? v - 2^t + 1 : v, added to the component's
 *              predictor.  AC: symbol run/size; 15/0 skips 16 coefficients, 0/0 ends the block; the value is extended like the
 *              DC difference.  Coefficients arrive in zig-zag order and are stored in natural order.
 *   IDCT       on coef * quant in int32, jpeg_idct_islow: CONST_BITS 13, PASS1_BITS 2, constants 2446 3196 4433 6270 7373 9633
 *              12299 15137 16069 16819 20995 25172, the even / odd butterfly; columns first, descaled (x + 2^10) >> 11, then
 *              rows, descaled (x + 2^17) >> 18 (arithmetic shifts), + 128, clamped to 0..255.
 *   4:2:0      chroma has dh = ceil(h/2) x dw = ceil(w/2) real samples s; the padding of the last MCU is never read.  dw > 2:
 *              output row 2r + v uses colsum[x] = 3 s[r][x] + s[r'][x], r' = max(r-1, 0) for v = 0, min(r+1, dh-1) for v = 1;
 *              out[2x] = (3 colsum[x] + colsum[x-1] + 8) >> 4, out[2x+1] = (3 colsum[x] + colsum[x+1] + 7) >> 4, at the edges
 *              out[0] = (4 colsum[0] + 8) >> 4, out[2dw-1] = (4 colsum[dw-1] + 7) >> 4.  dw <= 2: out[y][x] = s[y/2][x/2].
 *   colour     FIX(x) = int(x * 65536 + 0.5), cb' = cb - 128, cr' = cr - 128:  R = y + ((FIX(1.402) cr' + 32768) >> 16),
 *              B = y + ((FIX(1.772) cb' + 32768) >> 16), G = y + ((-FIX(0.34414) cb' + 32768 - FIX(0.71414) cr') >> 16), each
 *              clamped to 0..255.  Gray: R = G = B = y.
 *
 * t3d_jpeg_index (HOST ONLY: no HIP call, never initialises the GPU; every read is checked against `bytes`): fills *info, and
 * -- when segs != NULL -- one t3d_jpeg_seg per seg_mcus consecutive MCUs in scan order (the last may be ragged);
 * seg_capacity < nseg is T3D_ERR_ARG.  segs == NULL fills info only, nseg included.  seg_mcus >= 1.
 * An MCU is one 8x8 block per component (gray, 4:4:4) or 4 Y + Cb + Cr blocks = 16x16 pixels (4:2:0). */
enum { T3D_JPEG_GRAY = 0, T3D_JPEG_444 = 1, T3D_JPEG_420 = 2 };
enum { T3D_JPEG_REASON_NONE = 0,
       T3D_JPEG_REASON_SOF = 1,          /* progressive, extended, lossless or arithmetic-coded frame */
       T3D_JPEG_REASON_PRECISION = 2,    /* sample precision other than 8 bit */
       T3D_JPEG_REASON_RESTART = 3,      /* DRI with a non-zero interval */
       T3D_JPEG_REASON_SAMPLING = 4,     /* 4:2:2, 4:4:0 or any other sampling */
       T3D_JPEG_REASON_COMPONENTS = 5,   /* 2, 4 or more components */
       T3D_JPEG_REASON_SCANS = 6,        /* more than one scan */
       T3D_JPEG_REASON_QUANT16 = 7,      /* a 16-bit quantisation table */
       T3D_JPEG_REASON_COLOURSPACE = 8   /* three components that are not YCbCr (Adobe transform 0, ids 'R' 'G' 'B') */ };
typedef struct {
  int h, w, ncomp, sampling;             /* T3D_JPEG_GRAY / _444 / _420 */
  int mcus_x, mcus_y;                    /* the MCU grid */
  int seg_mcus, nseg;                    /* nseg = ceil(mcus_x * mcus_y / seg_mcus) */
  long long scan_offset, scan_bytes;     /* the entropy-coded bytes (stuffed) within the file, up to the marker behind them */
  int reason, reserved;                  /* T3D_JPEG_REASON_* when the call returned T3D_ERR_UNSUPPORTED */
  unsigned char comp_dc[4], comp_ac[4];  /* component -> index into dc_* / ac_* */
  unsigned char quant[3][64];            /* per component, natural (row-major) order */
  unsigned char dc_bits[2][16], dc_vals[2][16];     /* DHT: codes per length 1..16, then the symbols in code order */
  unsigned char ac_bits[2][16], ac_vals[2][256];
} t3d_jpeg_info;                         /* 864 bytes */
typedef struct {
  unsigned int byte;                     /* the MCU's first bit lies in this byte of the stuffed scan (offset from scan_offset; */
  short pred[3];                         /*   never a stuffed 00) ...   the DC predictor of each component at that point        */
  unsigned char bit, reserved;           /* ... at this bit, 0 = the most significant                                           */
  int mcu;                               /* index of the segment's first MCU (= segment index * seg_mcus)                       */
} t3d_jpeg_seg;                          /* 16 bytes */
int t3d_jpeg_index(const unsigned char* data, long long bytes, int seg_mcus, t3d_jpeg_info* info, t3d_jpeg_seg* segs,
                   long long seg_capacity);

/* t3d_jpeg_decode_u8: B indexed files -> packed RGB uint8 [h][w][3] per image (what collate_frames packs), FIVE enqueues on
 * `stream` whatever B is (memsets of the coefficients and of status, then the entropy, IDCT and colour kernels); no allocation, no host
 * synchronisation, no read-back.  All tables in DEVICE memory:
 *   data [data_bytes]      the files' bytes, image i at items[i].file_offset, file_bytes long
 *   infos [B], segs [total_segs] (image i's nseg entries from items[i].seg_offset on), items [B]
 *   out [out_bytes]        image i at items[i].out_offset (64 bit, any alignment: dword stores where the address allows)
 *   work [work_bytes]      t3d_jpeg_decode_work_bytes(total_blocks) bytes, 16-byte aligned: int16 [total_blocks][64] quantised
 *                          coefficients, then uint8 [total_blocks][64] samples; image i owns the blocks from items[i].block_offset
 *                          on, mcus_x * mcus_y * (1, 3 or 6) of them
 *   status int32 [B]       0: decoded to the last MCU; 1: a lane met a code that does not exist and left the rest of its
 *                          segment's blocks zero; 2: the record is inconsistent (an info the indexer would not write, a range
 *                          outside data / segs / out / work) -- nothing of that image is read or written
 *   max_segs, max_blocks   upper bounds of one image's nseg and block count: they size the grids; the kernels loop, so a bound
 *                          that is too small costs time, not correctness
 * Memory safety does not depend on the stream: every read of it is clamped to the image's scan, at a marker or the scan's
 * end the reader feeds zero bits and does not advance, a lane decodes at most seg_mcus MCUs of at most 64 coefficients a
 * block and writes only its own segment's blocks.
 * T3D_ERR_ARG, nothing launched: a NULL pointer, B < 0 or > 65535, negative or zero totals, work misaligned or work_bytes below
 * the query, out_bytes <= 0.  B == 0 returns T3D_OK and launches nothing. */
typedef struct {
  long long file_offset, file_bytes;     /* within data */
  long long out_offset;                  /* within out */
  long long block_offset;                /* within work, in 8x8 blocks */
  long long seg_offset;                  /* within segs */
  long long reserved;
} t3d_jpeg_item;                         /* 48 bytes */
int t3d_jpeg_decode_work_bytes(long long total_blocks, long long* bytes);
int t3d_jpeg_decode_u8(const unsigned char* data, long long data_bytes, const t3d_jpeg_info* infos, const t3d_jpeg_seg* segs,
                       long long total_segs, const t3d_jpeg_item* items, unsigned char* out, long long out_bytes, void* work,
                       long long work_bytes, long long total_blocks, int* status, int B, int max_segs, int max_blocks,
                       void* stream);

/* t3d_jpeg_decode_roi_u8: of each of B indexed files ONE PIXEL RECTANGLE [x0, x1) x [y0, y1) -> packed RGB uint8
 * [y1 - y0][x1 - x0][3] at the item's out_offset: what Objectron.crop slices out of the decoded frame and collate_crops packs,
 * so t3d_augment_crops_u8, its chain variant and the cache fill read it through the same (offset, h, w) descriptor.
 * DEFINITION: the pixels are those t3d_jpeg_decode_u8 writes for the same file, sliced [y0:y1, x0:x1], bit for bit -- the
 * definition above (islow IDCT, fancy 4:2:0 upsampling with its edge rules on the REAL image's dh, dw, the 16.16 colour
 * constants) plus the slice.  Only the work differs: entropy decoding of the segments that own an MCU the rectangle reads, each
 * once (inside such a segment the MCUs outside are parsed -- bits and DC predictors advance -- and not stored), the IDCT of the
 * rectangle's blocks, the colour conversion of the rectangle's pixels.  The same FIVE enqueues whatever B is; no allocation, no
 * host synchronisation, no read-back.
 *   MCU rectangle [mx0, mx1) x [my0, my1), computed by the caller and checked here: it must hold every block the rectangle's
 *     pixels read.  Gray, 4:4:4: the pixels' own MCUs, x >> 3, y >> 3.  4:2:0: pixel (y, x) reads chroma rows y >> 1 and
 *     (y >> 1) - 1 (y even) / + 1 (y odd) and chroma columns x >> 1 and (x >> 1) - 1 (x even) / + 1 (x odd), clamped to
 *     [0, dh - 1] / [0, dw - 1] -- the rectangle halved and dilated by the one sample its edge pixels reach for; chroma sample s
 *     lies in MCU s >> 3 (which covers the luma).  dw <= 2: libjpeg replicates, no dilation.  A larger rectangle is accepted.
 *   infos [B]              the files' t3d_jpeg_info (scan_offset is not used here: the items say where the bytes are)
 *   items [B]              t3d_jpeg_item read this way: file_offset, file_bytes: where in `data` the item's uploaded bytes of the
 *                          SCAN lie and how many there are; reserved: the byte of the scan (offset from scan_offset) they begin
 *                          at -- the whole scan is (file's offset + scan_offset, scan_bytes, 0); out_offset (any alignment: a lane
 *                          stores dwords where its own address allows, bytes otherwise); block_offset, in 8x8 blocks; seg_offset
 *   rects int32 [B][12]    x0 y0 x1 y1  mx0 my0 mx1 my1  seg_first seg_count  0 0: segs[seg_offset + k] is the file's segment
 *                          seg_first + k, k < seg_count; the uploaded segments must include the first and the last the MCU
 *                          rectangle needs, those of MCU (my0, mx0) and MCU (my1 - 1, mx1 - 1)
 *   work [work_bytes]      t3d_jpeg_decode_work_bytes(total_blocks) bytes, 16-byte aligned, total_blocks the sum over the items
 *                          of (mx1 - mx0) * (my1 - my0) * (1, 3 or 6): COMPACT, blocks exist for the MCU rectangles only
 *   Partial data: the reader treats every byte outside the uploaded span as the end of the scan -- it feeds zero bits and does
 *     not advance.  The span from the byte of the first needed segment to the byte of the segment behind the last needed one,
 *     plus 8 bytes (the window reads ahead), decodes like the whole scan.
 *   status int32 [B]       0: decoded; 1: a lane met a code that does not exist (or its segment begins outside the uploaded
 *                          bytes) and left the rest of its segment zero; 2: the record is inconsistent (an info the indexer would
 *                          not write, an empty rectangle or one outside the image, an MCU rectangle outside the grid or not
 *                          holding the blocks the pixels read, uploaded segments that miss a needed one, a range outside data /
 *                          scan / segs / out / work) -- nothing of that item is read or written
 *   max_lanes, max_blocks, max_runs   upper bounds over the items of (my1 - my0) * ((mx1 - mx0 - 1) / seg_mcus + 2), of the
 *                          MCU rectangle's block count and of (y1 - y0) * ceil((x1 - x0) / 4): they size the grids; the kernels
 *                          loop, so a bound that is too small costs time, not correctness
 * Memory safety as above: every per-item range is checked by every kernel before use, every stream read is clamped to the
 * uploaded bytes, a block ends at coefficient 63, a lane writes only blocks of its own segment that lie in the rectangle.
 * T3D_ERR_ARG, nothing launched: as t3d_jpeg_decode_u8, and rects NULL or a bound below 1.  B == 0 returns T3D_OK. */
int t3d_jpeg_decode_roi_u8(const unsigned char* data, long long data_bytes, const t3d_jpeg_info* infos, const t3d_jpeg_seg* segs,
                           long long total_segs, const t3d_jpeg_item* items, const int* rects, unsigned char* out,
                           long long out_bytes, void* work, long long work_bytes, long long total_blocks, int* status, int B,
                           long long max_lanes, int max_blocks, long long max_runs, void* stream);

/* t3d_detect_roi_plan: the join of t3d_detect_draw and t3d_jpeg_decode_roi_u8 ON THE DEVICE, one launch, no read-back
 * (csrc/detect_roi.hip, csrc/detect_roi.h; torchdet3d/dataloaders/detection_arena.py, crop_decode).  t3d_detect_draw reads no
 * pixel, so it can run BEFORE the decode; this call turns its records into the rectangle decode's tables, so that only the part
 * of each frame that its crop reads is decoded, and rewrites the records so that t3d_detect_augment_u8, unchanged, makes the same
 * image from the part as from the whole frame, bit for bit.
 * t3d_detect_roi_plan_host is the same arithmetic on the CPU: the same arguments, every pointer a HOST pointer, `stream`
 * ignored; HOST ONLY, no HIP call, never initialises the GPU.  tests/test_detect_roi_plan_host.py holds it to numpy.
 *   records [B] t3d_det_sample, IN AND OUT: the planned samples' records are rewritten in place, every other one is not touched
 *   sample int32 [n]       item j belongs to record sample[j], each record at most once (NULL: item j to record j); an index
 *                          outside [0, B) plans the whole frame
 *   infos [n], items [n]   the frames' t3d_jpeg_info rows and the WHOLE-FRAME t3d_jpeg_item of t3d_jpeg_decode_u8 (file_offset:
 *                          the file; seg_offset: its first segment; out_offset, block_offset: prefix sums of whole frames)
 *   src_bytes              the size of the buffer the frames are decoded into (t3d_detect_augment_u8's src_bytes)
 *   roi_items [n], rects int32 [n][12], diag int32 [n][2]: OUT
 * The source rectangle is the crop intersected with the pasted frame, turned back to source pixels.  With (rw, rh) the turned frame -- (w, h) for
 * turns 0, (h, w) for turns 1 and 3 -- a0 = max(cx0 - left, 0), a1 = min(cx1 - left, rw), b0 = max(cy0 - top, 0),
 * b1 = min(cy1 - top, rh):
 *     turns 0: x in [a0, a1), y in [b0, b1)     turns 1: x in [w - b1, w - b0), y in [a0, a1)
 *     turns 3: x in [b0, b1), y in [h - a1, h - a0)
 * exactly, no slack: the bilinear taps of t3d_detect_augment_u8 never leave [cx0, cx1 - 1] x [cy0, cy1 - 1].  An empty
 * intersection (a crop wholly in the fill) gives (0, 0, 1, 1).
 *   rects row     x0 y0 x1 y1, the MCU rectangle the decode's own rule gives for it (csrc/jpeg_decode.h: roi_mcus),
 *                 seg_first = (my0 * mcus_x + mx0) / seg_mcus, seg_count up to segment ((my1 - 1) * mcus_x + mx1 - 1) / seg_mcus, 0 0
 *   item          file_offset + scan_offset, scan_bytes, reserved 0 (the whole scan, which is resident); seg_offset + seg_first;
 *                 out_offset and block_offset COPIED: the part lies packed at the start of its frame's slot and its blocks at the
 *                 start of its frame's share of the workspace, so no sum over the batch is needed and the host's whole-frame
 *                 totals and bounds remain upper bounds of the decode call
 *   record        offset = out_offset; h, w = the rectangle's; (left, top) += (x0, y0) for turns 0, (y0, w - x1) for turns 1,
 *                 (h - y1, x0) for turns 3, with the ORIGINAL h, w (saturated at 2^31 - 1): the part lies where it lay in the
 *                 canvas; every other field stays
 *   diag          the rectangle's pixels and the MCU rectangle's 8x8 blocks (saturated at 2^31 - 1)
 * A record that t3d_detect_augment_u8 would refuse (judged with src_bytes), one whose h, w are not the info's, or a missing one
 * is NOT rewritten and gets the whole frame: that sample behaves as without this call.  An info row whose h, w, sampling,
 * MCU grid or seg_mcus the indexer would not write gets the whole-frame tables as they stand and diag (0, 0);
 * t3d_jpeg_decode_roi_u8 refuses it (status 2).  Every range written here is checked again there and by t3d_detect_augment_u8 before anything is read.
 * One sample a lane.  T3D_ERR_ARG, nothing launched: B or n < 0 or > 65535, src_bytes < 0, with n > 0 a NULL pointer (but
 * sample).  n == 0 returns T3D_OK. */
int t3d_detect_roi_plan(void* records, int B, const int* sample, const t3d_jpeg_info* infos, const t3d_jpeg_item* items, int n,
                        long long src_bytes, t3d_jpeg_item* roi_items, int* rects, int* diag, void* stream);
int t3d_detect_roi_plan_host(void* records, int B, const int* sample, const t3d_jpeg_info* infos, const t3d_jpeg_item* items, int n,
                             long long src_bytes, t3d_jpeg_item* roi_items, int* rects, int* diag, void* stream);

/* The MCU index BUILT ON THE DEVICE (csrc/jpeg_scan.h, csrc/jpeg_scan.hip): for a frame nobody has indexed -- a video or camera
 * frame -- the host reads only the markers (t3d_jpeg_header) and the device finds the MCU starts and DC predictors of every
 * frame of a batch (t3d_jpeg_index_device).  The rows are t3d_jpeg_index's, byte for byte; t3d_jpeg_decode_u8 runs behind it
 * unchanged.
 *
 * t3d_jpeg_header (HOST ONLY like t3d_jpeg_index: no HIP call; every read is checked against `bytes`): the marker half of
 * t3d_jpeg_index and nothing of the scan.  The same return codes and the same info->reason for every file the markers refuse
 * (a Huffman table that is no prefix code included); *info as t3d_jpeg_index fills it, except that scan_bytes is the bytes from
 * scan_offset to the end of the file -- the clamp of every scan read, not yet the scan's length.
 *
 * DEFINITION of t3d_jpeg_index_device: infos[i].scan_bytes and image i's nseg rows of segs are what t3d_jpeg_index writes for
 * file i and infos[i].seg_mcus, `reserved` included, and status[i] == 0, exactly when t3d_jpeg_index returns T3D_OK for it.
 * METHOD.  Baseline Huffman streams self-synchronise.  The stuffed scan is cut into subsequences of sub_bytes raw bytes, one
 * lane each; a lane owns every symbol (a code plus its extra bits) whose first bit lies in its subsequence.  The state that
 * crosses a boundary: the next symbol's byte and bit (the convention of t3d_jpeg_seg), the block slot in the MCU, the next
 * zig-zag position, or "no valid state".  speculate: every lane decodes from its first byte as if an MCU began there (lane 0's
 * entry is true).  settle: every lane takes its predecessor's exit as its entry and decodes again where that changed, until no
 * lane changed -- then the chain is the sequential decode; at most nsub rounds whatever the data, only the time depends on how
 * fast the stream synchronises.  count: an exclusive scan per image of the MCU starts and the DC differences per component.
 * emit: every lane decodes once more with its true entry, MCU number and predictors, writes the rows of the MCUs it owns and
 * applies the host indexer's checks to everything before the end of the last MCU; the lane in which the last MCU ends checks
 * the trailer (the rest of the byte, fill FFs, FF D9).  What lies behind that point is never trusted.
 * FOUR kernels on `stream` whatever B is (speculate; settle + count, one workgroup per image, rounds separated by workgroup
 * barriers; emit; finish), no memset, no allocation, no host synchronisation, no read-back.  No workgroup waits for another.
 *   data [data_bytes]      the files' bytes, image i at items[i].file_offset, file_bytes long
 *   infos [B]  IN and OUT  as t3d_jpeg_header filled them.  scan_bytes is not read: the clamp is file_bytes - scan_offset.
 *                          On return scan_bytes is the scan's length (status 0) or -1 (status 1 or 2): t3d_jpeg_decode_u8
 *                          given these infos refuses such an image with its own status 2
 *   segs [total_segs] OUT  image i's nseg rows from items[i].seg_offset on; rows of an image with status 1 are unspecified
 *   items [B]              t3d_jpeg_item read this way: file_offset, file_bytes, seg_offset as for t3d_jpeg_decode_u8;
 *                          block_offset: the image's first SUBSEQUENCE RECORD in work (in records, not blocks), it owns
 *                          nsub = ceil((file_bytes - scan_offset) / sub_bytes) of them; out_offset and reserved are not read
 *   sub_bytes              4 .. 2^30 raw bytes of the stuffed scan a lane
 *   work [work_bytes]      t3d_jpeg_index_work_bytes(sum of the images' file_bytes - scan_offset, B, sub_bytes) bytes, 16-byte
 *                          aligned: B records of 32 bytes (one an image), then 32 bytes a subsequence
 *   status int32 [B] OUT   0: indexed.  1: a scan t3d_jpeg_index returns T3D_ERR_ARG for (no such code, a DC category above 11,
 *                          a run past coefficient 63, a predictor outside int16, a marker or the end of the data inside the
 *                          scan, no EOI behind it; a second scan, which t3d_jpeg_index calls unsupported, lands here too).
 *                          2: the record is inconsistent (an info the header would not write, a table that is no prefix code, a
 *                          range outside data / segs / work) -- nothing of that image's bytes, rows or records is read or
 *                          written
 *   max_subs               an upper bound of one image's nsub: it sizes the grids; the kernels loop, so a bound that is too
 *                          small costs time, not correctness
 * Memory safety does not depend on the stream: every read of it is clamped to the image's bytes, a decode step consumes at least
 * one bit or ends the lane, a lane ends at its subsequence's end, every row and record index is checked against the image's share.
 * T3D_ERR_ARG, nothing launched: a NULL pointer, B < 0 or > 65535, sub_bytes outside 4 .. 2^30, data_bytes or total_segs <= 0,
 * max_subs < 1, work misaligned or work_bytes below 32 * B.  B == 0 returns T3D_OK and launches nothing.
 * t3d_jpeg_index_work_bytes: T3D_ERR_ARG for bytes NULL, a negative total, B < 0 or > 65535, sub_bytes outside its range. */
int t3d_jpeg_header(const unsigned char* data, long long bytes, int seg_mcus, t3d_jpeg_info* info);
int t3d_jpeg_index_work_bytes(long long total_scan_bytes, int B, int sub_bytes, long long* bytes);
int t3d_jpeg_index_device(const unsigned char* data, long long data_bytes, t3d_jpeg_info* infos, t3d_jpeg_seg* segs,
                          long long total_segs, const t3d_jpeg_item* items, int sub_bytes, void* work, long long work_bytes,
                          int* status, int B, int max_subs, void* stream);

/* Baseline JPEG ENCODE on the device (csrc/jpeg_encode.h, csrc/jpeg_encode.hip): B RGB uint8 frames [B][h][w][3] of one size ->
 * B baseline JFIF files, the third leg beside t3d_jpeg_index and t3d_jpeg_decode_u8 (the files carry no restart markers: the
 * index accepts them with reason 0).  torchdet3d/utils/jpeg_encode.py wraps it, torchdet3d/utils/mjpeg.py puts the files into
 * a Motion-JPEG AVI (the reference's cv.VideoWriter, scripts/demo.py:50-54, 83-84).
 *
 * DEFINITION: libjpeg-turbo's default compression path as Pillow drives it, Image.save(format='JPEG', quality=q,
 * subsampling=s) with optimize and progressive off; restated in numpy by tests/jpeg_encode_ref.py.  The FILES are Pillow's on
 * libjpeg-turbo BYTE FOR BYTE (pinned by tests/test_jpeg_encode_host.py and tests/test_gpu_jpeg_encode.py).  Sampling is
 * T3D_JPEG_444 or T3D_JPEG_420; grey output, 4:2:2, optimised Huffman tables and restart intervals are out of scope.
 *   layout     SOI; APP0 FF E0 00 10 'JFIF\0' 01 01 00 00 01 00 01 00 00; two DQT, each FF DB 00 43, the id 0 / 1, 64 bytes in
 *              zig-zag order; SOF0 FF C0 00 11 08 hh hh ww ww 03 | 01 SS 00 | 02 11 01 | 03 11 01, SS = 22 (4:2:0) / 11 (4:4:4);
 *              four DHT in the order DC0 (00), AC0 (10), DC1 (01), AC1 (11): the Annex K tables (lengths 1F, B5, 1F, B5);
 *              SOS FF DA 00 0C 03 01 00 02 11 03 11 00 3F 00; the scan; FF D9.  The header is 623 bytes.
 *   quant      Annex K luminance / chrominance tables t, s = 5000 / q (q < 50) or 200 - 2q, entry = clip((t s + 50) / 100, 1,
 *              255) in integers, q = 1 .. 100.
 *   colour     jccolor, FIX(x) = int(x * 65536 + 0.5):  Y = (FIX(.299) R + FIX(.587) G + FIX(.114) B + 32768) >> 16,
 *              Cb = (-FIX(.16874) R - FIX(.33126) G + FIX(.5) B + (128 << 16) + 32767) >> 16,
 *              Cr = (FIX(.5) R - FIX(.41869) G - FIX(.08131) B + (128 << 16) + 32767) >> 16.
 *   edges      Y and 4:4:4 chroma: a real block's samples beyond the image replicate the last column and the last row.  4:2:0
 *              chroma: full-resolution columns are replicated to 16 ceil(w / 16), full-resolution rows only to even h; then
 *              (a + b + c + d + bias) >> 2 with bias 1 on even output columns, 2 on odd ones; then the last DOWNSAMPLED row is
 *              replicated down to 8 ceil(h / 16) rows (not the same as replicating full-resolution rows).
 *   FDCT       jfdctint.c (islow) on sample - 128 in int32, CONST_BITS 13, PASS1_BITS 2, FIX(x) = int(x * 8192 + 0.5) of
 *              0.298631336 0.390180644 0.541196100 0.765366865 0.899976223 1.175875602 1.501321110 1.847759065 1.961570560
 *              2.053119869 2.562915447 3.072711026; rows first -- outputs 0 and 4 are << 2, the rest (x + 2^10) >> 11 --, then
 *              columns -- outputs 0 and 4 are (x + 2) >> 2, the rest (x + 2^14) >> 15.
 *   quantise   d = 8 * table entry:  sign(c) * ((|c| + d / 2) / d).
 *   dummies    4:2:0 luma only: a block with block row >= ceil(h / 8) or block column >= ceil(w / 8) is not transformed; its
 *              AC coefficients are zero and its DC is that of the block before it in the MCU (a missing right block: its left
 *              neighbour; both blocks of a missing bottom row: the last block of the row above, real or dummy).
 *   entropy    one interleaved scan, MCUs in raster order, the DC difference of a component predicted across the whole scan;
 *              category + extra bits, ZRL (F0) for runs above 15, EOB (00) when the tail is zero; bits MSB first, a 00 behind
 *              every FF byte, the last byte padded with 1 bits.
 *
 * t3d_jpeg_encode_setup (HOST ONLY like t3d_jpeg_index: no HIP call): fills *out -- the header bytes, the divisors, the four
 * Huffman code tables, the geometry.  T3D_ERR_ARG: out NULL, h or w outside 1 .. 65535, quality outside 1 .. 100, a sampling
 * other than T3D_JPEG_444 / T3D_JPEG_420.
 * t3d_jpeg_encode_work_bytes: the work buffer of one call with these arguments.  T3D_ERR_ARG: bytes NULL, B < 0 or > 65535, h,
 * w, sampling as above, seg_mcus < 1, cap_bytes below header + 2 (625) or above 2^40.
 * t3d_jpeg_encode_u8: ONE memset and SEVEN kernels on `stream` whatever B is; no allocation, no host synchronisation, no
 * read-back; the same bytes on every run (integer arithmetic; lanes that share a 32-bit word of the stream OR their bits in).
 *   transform  a lane per 8x8 block: colour, edge rule, downsample, FDCT, quantise -> int16 [block in scan order][64 in
 *              zig-zag order]; the dummy blocks are written here (their DC needs only the sum of the source block's samples)
 *   count      a lane per SEGMENT of seg_mcus consecutive MCUs (as the decoder's lanes are cut): the exact bit length of its
 *              codes, DC predictors read from the coefficient array by index; then a per-frame exclusive scan
 *   emit       the same walk writes the codes at the segment's bit offset into the zeroed unstuffed stream
 *   stuffing   FF bytes counted per 64-byte chunk, the counts scanned per frame (that launch also writes the header, the
 *              EOI and the frame's result row), then the chunks scattered behind the header with the 00 bytes inserted
 *   frames     device, uint8 [B][h][w][3] contiguous
 *   tables     the struct t3d_jpeg_encode_setup filled, in HOST memory: the call reads the geometry from it (grid sizes and the
 *              argument checks need it without a read-back); tables_dev: a copy of the same struct in DEVICE memory, from
 *              which the kernels read the divisors, the code tables and the header.  Every index and range the kernels use
 *              comes from the host copy, so memory safety does not depend on the device copy.
 *   out        device, frame i's file at out + i * cap_bytes; results [B] device: bytes = the file's length, overflow = 0; or,
 *              when the file does not fit cap_bytes or its unstuffed scan does not fit its share of work (cap_bytes rounded up
 *              to 64), overflow = 1 and bytes = header + unstuffed scan + 2, a lower bound of the need -- stuffing at most
 *              doubles the scan, so a slot of 2 * bytes always suffices.  An overflowing frame writes nothing outside its own
 *              slot and every other frame of the call is unaffected.
 *   work       device, 16-byte aligned, t3d_jpeg_encode_work_bytes bytes
 * T3D_ERR_ARG, nothing launched: a NULL pointer, B < 0 or > 65535, tables not one that setup fills, out or work not 16-byte
 * aligned, seg_mcus < 1, cap_bytes below header + 2, work_bytes below the query.  B == 0 returns T3D_OK and launches nothing. */
typedef struct t3d_jpeg_enc_tables {
  int h, w, quality, sampling;           /* T3D_JPEG_444 / T3D_JPEG_420 */
  int mcus_x, mcus_y, mcu_blocks, blocks;        /* the MCU grid, 3 or 6 blocks an MCU, blocks of a frame */
  int luma_rows, luma_cols;              /* ceil(h / 8), ceil(w / 8): luma blocks beyond them are dummies (4:2:0) */
  int header_bytes, reserved;
  unsigned short divisor[2][64];         /* 8 * quantisation entry, natural (row-major) order; luminance, chrominance */
  unsigned int huff[4][256];             /* DC 0, DC 1, AC 0, AC 1 by symbol: code length << 16 | code; 0: no such symbol */
  unsigned char header[640];             /* SOI .. SOS, header_bytes of them */
} t3d_jpeg_enc_tables;
typedef struct t3d_jpeg_enc_result {
  long long bytes;
  int overflow, reserved;
} t3d_jpeg_enc_result;
int t3d_jpeg_encode_setup(int h, int w, int quality, int sampling, t3d_jpeg_enc_tables* out);
int t3d_jpeg_encode_work_bytes(int B, int h, int w, int sampling, int seg_mcus, long long cap_bytes, long long* bytes);
int t3d_jpeg_encode_u8(const unsigned char* frames, int B, const t3d_jpeg_enc_tables* tables,
                       const t3d_jpeg_enc_tables* tables_dev, int seg_mcus, unsigned char* out, long long cap_bytes,
                       t3d_jpeg_enc_result* results, void* work, long long work_bytes, void* stream);

/* Materialise a block output:  z = act(scale*y + shift) + residual   (residual may be NULL; scale NULL = identity).
 * Replaces the BatchNorm normalise pass + `x + self.conv(x)` (mobilenetv3.py:159,162-164). y,z,residual [M,C]. */
int t3d_bn_apply(int dtype, const void* y, const t3d_prologue* pro, const void* residual, void* z, int M, int C,
                 void* stream);

/* Backward of t3d_bn_apply's activation:  dzp = dz * act'(scale*y + shift);
 * stats [2*C] fp64 += sum(dzp), sum(dzp*y) (caller zeroes). */
int t3d_bn_act_bwd(int dtype, const void* dz, const void* y, const t3d_prologue* pro, void* dzp, double* stats,
                   int M, int C, void* stream);

/* Global average pool of the activated last feature map (model_builder.py:96-110, mode 'avg'):
 *   pooled[b][c] = mean_hw act(scale*y + shift),  y [B,HW,C] raw (dtype), pooled [B,C] fp32. */
int t3d_gap_fwd(int dtype, const void* y, const t3d_prologue* pro, float* pooled, int B, int HW, int C,
                void* stream);

/* Every pooling mode of ModelWrapper._glob_feature_vector (model_builder.py:96-110): 'avg' (as t3d_gap_fwd), 'max'
 * (F.adaptive_max_pool2d(x, 1)) and 'avg+max' (their sum).  argmax [B,C] int32 receives the (h*W + w) position of
 * each maximum -- the first one in scan order among equal values, which is where PyTorch's backward routes the
 * gradient -- and is what t3d_pool_bwd reads back (may be NULL for T3D_POOL_AVG).
 * Backward: dz [B,HW,C] (dtype) = the pooled gradient routed back (T3D_POOL_AVG: dpooled[b][c]/HW at every pixel)
 * * act'(scale*y + shift); stats [2*C] fp64 += sum(dz), sum(dz*y). */
enum { T3D_POOL_AVG = 0, T3D_POOL_MAX = 1, T3D_POOL_AVGMAX = 2 };
int t3d_pool_fwd(int dtype, const void* y, const t3d_prologue* pro, int mode, float* pooled, int* argmax, int B,
                 int HW, int C, void* stream);
int t3d_pool_bwd(int dtype, const float* dpooled, const void* y, const t3d_prologue* pro, int mode, const int* argmax,
                 void* dz, double* stats, int B, int HW, int C, void* stream);

/* Regression + class heads (ModelWrapper.forward, model_builder.py:126-146):
 *   f' = act(scale*f + shift)                       (classifier BatchNorm1d + h_swish, or identity: pro NULL)
 *   kp[b]     = sigmoid(Wreg[cats[b]] f'[b] + breg[cats[b]])      [B,18]   (:137-139, class-gathered GEMV)
 *   logits[b] = Wcls (f'[b] * mask[b]) + bcls                     [B,ncls] (:142; mask = Dropout(0.5) keep/scale
 *               factors {0,2}, NULL in eval mode); logits may be NULL (num_classes == 1, :144).
 * f [B,F] fp32, Wreg [9,18,F], breg [9,18], Wcls [ncls,F], cats int64 [B]. */
int t3d_head_fwd(const float* f, const t3d_prologue* pro, const int64_t* cats, const float* wreg,
                 const float* breg, const float* wcls, const float* bcls, const float* mask, float* kp,
                 float* logits, int B, int F, int ncls, void* stream);

/* Export-mode heads (ModelWrapper.forward_to_onnx, model_builder.py:112-124): EVERY one of the 9 regressors applied
 * to every sample in one launch, kp_all [9,B,18] = sigmoid(Wreg[k] f'[b] + breg[k]); logits as above (eval: no mask). */
int t3d_head_fwd_all(const float* f, const t3d_prologue* pro, const float* wreg, const float* breg, const float* wcls,
                     const float* bcls, float* kp_all, float* logits, int B, int F, int ncls, void* stream);

/* A single head applied on its own -- `model.regressors[k](f)` / `model.cls_fc[1](f)` for callers that use the
 * reference's attributes directly (model_builder.py:79-85): y [M,N] = x [M,K] w[N,K]^T + bias, fp32, any N. */
int t3d_linear_fwd(const float* x, const float* w, const float* bias, float* y, int M, int K, int N, void* stream);

/* Head backward.  dkp [B,18], dlogits [B,ncls] (may be NULL) -> df [B,F] (when pro is given: the gradient
 * at the BatchNorm1d OUTPUT, i.e. already multiplied by act'; then stats [2*F] fp64 += sum(df), sum(df*f)),
 * dwreg [9,18,F], dbreg [9,18], dwcls [ncls,F], dbcls [ncls] are ACCUMULATED (+=, batch slices in parallel): the
 * caller zeroes them once per step, like every other weight-gradient buffer of this ABI.
 * dpre [B,18] fp32 scratch. */
int t3d_head_bwd(const float* f, const t3d_prologue* pro, const int64_t* cats, const float* wreg,
                 const float* wcls, const float* mask, const float* kp, const float* dkp, const float* dlogits,
                 float* dpre, float* df, double* stats, float* dwreg, float* dbreg, float* dwcls, float* dbcls,
                 int B, int F, int ncls, void* stream);
/* The weight / bias gradients of t3d_head_bwd on their own: pass dwreg = NULL there (data gradient only, dpre is left
 * behind) and issue this on the weight-gradient stream -- 44 us off the start of the backward's critical chain. */
int t3d_head_bwd_weights(const float* f, const t3d_prologue* pro, const int64_t* cats, const float* mask, const float* dpre,
                         const float* dlogits, float* dwreg, float* dbreg, float* dwcls, float* dbcls, int B, int F, int ncls,
                         void* stream);

/* Keypoint / class losses of torchdet3d/losses/regression_losses.py + builders/loss_builder.py:7-28,
 * combined as LossManager.parse_losses does (:79-95), value AND gradient in one launch, plus the
 * training metrics of evaluation/metrics.py:10-37.  A coefficient of 0 disables a term.
 *   total = lam_reg * sum_i c_i * L_i(kp, gt)  +  lam_cls * c_ce * CE(logits, cats)
 * out[0] total, out[1] sum_i c_i L_i, out[2] c_ce*CE, out[3] ADD (mean), out[4] SADD (mean), out[5] accuracy,
 * out[6] sum ADD / 9 ... (metrics with reduce_mean=False: out[6] ADD, out[7] SADD, out[8] correct count).
 * dkp [B,18] / dlogits [B,ncls] (may be NULL: values only) receive d total / d input. */
typedef struct {
  float c_l1, c_mse, c_smoothl1, smoothl1_beta, c_add, c_diag, c_wing, wing_w, wing_eps, c_ce;
  float lam_reg, lam_cls;
} t3d_loss_cfg;
int t3d_loss_fwd_bwd(const t3d_loss_cfg* cfg, const float* kp, const float* gt_kp, const float* logits,
                     const int64_t* cats, float* out, float* dkp, float* dlogits, int B, int ncls, void* stream);

/* Per-sample summands of the validation metrics (torchdet3d/evaluation/metrics.py:39-68 `compute_metrics_per_cls`, which
 * calls compute_average_distance / compute_accuracy with reduce_mean=False on every class subset, :48-55):
 * out [B][3] = { sum_k ||p_k - t_k|| / 9, symmetric-ADD summand / 9 (:13-21), arg-max hit (:31-37; logits NULL: the
 * width-1 "targets" of num_classes == 1, arg-max always 0) } -- the host adds them per class: one launch and one
 * read-back per validation batch instead of two launches and two syncs per class present. */
int t3d_metrics_per_sample(const float* kp, const float* gt_kp, const float* logits, const int64_t* cats, float* out,
                           int B, int ncls, void* stream);

/* 2-D based 3-D IoU of the validation loop, batched on the device (torchdet3d/evaluation/metrics.py:70-89 with
 * torchdet3d/utils/geometry.py:51-108 `lift_2d(..., portrait)` and the objectron box fit + box-box IoU it calls):
 *   pred_kp, gt_kp [B,9,2] fp32 normalised keypoints (the centre keypoint 0 is not used by the lift, :71-72);
 *   camera_ndc: NULL for the default camera (geometry.py:16-19,29-37: fx = fy = 2, cx = cy = 0) or {fx, fy, cx, cy} fp64 (HOST);
 *   iou [B] fp64 per-sample IoU (0 where the reference swallows a QhullError / LinAlgError, metrics.py:82-86), may be
 *   NULL when only `lifted` is wanted; total: fp64 scalar += sum(iou) (may be NULL; caller zeroes);
 *   lifted [B,2,9,3] fp64 or NULL: the lifted vertices of (pred, gt) -- what lift_2d returns. */
int t3d_iou3d(const float* pred_kp, const float* gt_kp, int B, int portrait, const double* camera_ndc, double* iou,
              double* total, double* lifted, void* stream);

/* The box-box part alone: verts [B,2,9,3] fp64 = B pairs of 9-vertex boxes in objectron's vertex order (centre, then
 * the 8 corners), as `box.Box(vertices)` takes them (metrics.py:79-81) -> iou [B] fp64. */
int t3d_box_iou3d(const double* verts, int B, double* iou, double* total, void* stream);

/* Squeeze-excite gate (SELayer, mobilenetv3.py:92-107) from the depthwise kernel's per-sample sums, all fp32, C, R <= 1024:
 *   m = scale*gap_sum/HW + shift (= mean_hw of the BatchNorm output), h = relu(W1 m + b1), q = W2 h + b2, s = h_sigmoid(q).
 * _fwd_fused (two launches, one per product): gap_sum [B,C] (float sums; int64 fixed point after t3d_set_exact_pool(1)),
 *   scale, shift [C], b1 [R], b2 [C] -> m, q, s [B,C], h [B,R].  It takes TRANSPOSED copies of the FC weights, so that its
 *   contractions read [input][output] like the backward's: w1t [C,R] = W1^T, w2t [R,C] = W2^T for the parameters W1 [R,C]
 *   (fc.0.weight) and W2 [C,R] (fc.2.weight); the caller keeps them current, e.g. with t3d_pack_weights_batched(T3D_F32, ...).
 * _bwd_data (two launches): ps_stats [B,C,2] = per-sample P1 = sum_hw(dv), P2 = sum_hw(dv*y) from t3d_pwconv_dgrad (dv:
 *   gradient at the gated tensor, y: raw depthwise output); gap_sum, scale, shift as in the forward; w1 [R,C], w2 [C,R]: the
 *   parameters THEMSELVES; h, q, s: what the forward left.  With ds = scale*P2 + shift*P1 it writes
 *   dq [B,C] = h_sigmoid'(q) ds, dp [B,R] = relu'(h) (dq W2) and g [B,C] = (dp W1) / HW, the pooled path's per-pixel gradient
 *   (du = s*dv + g), and accumulates the depthwise BatchNorm's backward sums stats [2*C] fp64 += sum(du), sum(du*y) -- stats
 *   may be NULL, and is spread over the reduction replicas of t3d_set_reduction_replicas like the conv kernels' sums.
 * _bwd_weights OVERWRITES the FC gradients dw1 [R,C], db1 [R], dw2 [C,R], db2 [C] from m, h and the dq, dp that _bwd_data
 *   (or t3d_se_after_bwd) left -- leaves of the backward graph, issued on the weight-gradient stream. */
int t3d_se_fwd_fused(const float* gap_sum, const float* scale, const float* shift, const float* w1t, const float* b1,
                     const float* w2t, const float* b2, float* m, float* h, float* q, float* s, int B, int C, int R, int HW,
                     void* stream);
int t3d_se_bwd_data(const float* ps_stats, const float* gap_sum, const float* scale, const float* shift, const float* w1,
                    const float* w2, const float* h, const float* q, const float* s, float* g, float* dq, float* dp,
                    double* stats, int B, int C, int R, int HW, void* stream);
int t3d_se_bwd_weights(const float* m, const float* h, const float* dq, const float* dp, float* dw1, float* db1, float* dw2,
                       float* db2, int B, int C, int R, void* stream);

/* Squeeze-excite applied AFTER the activation (the no-expand block layout, mobilenetv3.py:138-140: dw -> BN -> act ->
 * SE -> 1x1; MobileNetV3-small features.1): v = s*a, a = act(scale*y + shift).  Forward: t3d_gap_fwd gives mean_hw(a),
 * t3d_se_fwd_fused (scale = 1, shift = 0, HW = 1) the gate.  Backward, with dv [B*HW,C] the gradient at the gated tensor:
 *   _sums : ps [B,C,2] = { sum_hw dv*a, 0 }   -> t3d_se_bwd_data with scale = 0, shift = 1 (so that ds = ps[..][0]) gives g
 *   _apply: du = (s*dv + g) * act'(scale*y + shift) at the BatchNorm output, stats [2*C] fp64 += sum(du), sum(du*y). */
int t3d_se_after_sums(int dtype, const void* dv, const void* y, const t3d_prologue* pro, float* ps, int B, int HW, int C,
                      void* stream);
int t3d_se_after_apply(int dtype, const void* dv, const void* y, const t3d_prologue* pro, const float* s, const float* g,
                       void* du, double* stats, int B, int HW, int C, void* stream);

/* The same backward as ONE launch (t3d_se_after_sums -> t3d_se_bwd_data with scale = 0, shift = 1, no stats ->
 * t3d_se_after_apply).  The gate's input gradient g[b,:] depends only on sample b's own sums and on the two FC matrices,
 * so a workgroup owns a whole sample: it walks the sample's plane once for sum_hw dv*a, runs the two small mat-vecs
 * (w1 [R,C], w2 [C,R], fp32, read in their natural [I][O] orientation), then walks the plane a second time -- out of
 * cache, not HBM -- for du and the BatchNorm sums.  h [B,R], q, s [B,C]: what the forward's t3d_se_fwd_fused left
 * (the gate's input is mean_hw a, so g = dL/dm / HW).  Leaves g, dq [B,C], dp [B,R] for
 * t3d_se_bwd_weights; du [B*HW,C] in the storage dtype; stats [2*C] fp64 += sum(du), sum(du*y), replica
 * (workgroup % replicas) as set by t3d_set_reduction_replicas (may be NULL).  C % 8 == 0, C <= 1024, R <= 1024. */
int t3d_se_after_bwd(int dtype, const void* dv, const void* y, const t3d_prologue* pro, const float* w1, const float* w2,
                     const float* h, const float* q, const float* s, float* g, float* dq, float* dp, void* du,
                     double* stats, int B, int HW, int C, int R, void* stream);

/* t3d_bn_apply + t3d_pwconv_fwd in one launch: the 1x1 conv whose input is the previous block's OUTPUT, still in its raw
 * form (models/mobilenetv3.py:158-166: `x + conv(x)` feeding the next block's expansion).  The operand
 *   z = round_to_storage(act(scale*y_in + shift) + residual)
 * is formed on load exactly as t3d_bn_apply would have stored it, used for the contraction, and written to z_out once
 * (the skip connection and the backward need it).  bf16 streaming kernel; other cases run the two launches.
 *   y_in [M,K] raw, pro_in: its BatchNorm affine (+ activation), residual [M,K] or NULL, z_out [M,K],
 *   w [N,K], y [M,N] raw output, stats as in t3d_pwconv_fwd. */
int t3d_pwconv_fwd_mat(int dtype, const void* y_in, const t3d_prologue* pro_in, const void* residual, void* z_out,
                       const void* w, void* y, double* stats, int M, int HW, int K, int N, void* stream);

/* SSD detector post-processing (configs/detection/mnv2_ssd_300_2_heads.py:15-39,65-69: SSDHead outputs of <= 2 feature
 * maps -> DeltaXYWH decode -> softmax -> per-class greedy NMS), one launch per frame batch.  The implementing mmdetection
 * fork is external to the reference (README.md:56-57): arithmetic per the published mmdet definitions, parity unpinned.
 *   cls[l] [B*hw[l]][cls_stride[l]]: logits, channel = anchor*(num_classes+1) + class, background LAST;
 *   reg[l] [B*hw[l]][reg_stride[l]]: deltas, channel = anchor*4 + (dx, dy, dw, dh); storage dtype;
 *   anchors [sum hw*nanchors][4] fp32 (x1, y1, x2, y2 in input pixels), level-major, then pixel, then anchor;
 *   stds [4]; boxes are clipped to (img_w, img_h).
 *   out [B][num_classes][max_per_class][6] = x1, y1, x2, y2, score, label in NMS order; counts [B][num_classes].
 * cls / reg / hw / nanchors / *_stride are HOST arrays of length nlevels. */
int t3d_ssd_decode_nms(int dtype, int nlevels, const void* const* cls, const void* const* reg, const int* hw,
                       const int* nanchors, const int* cls_stride, const int* reg_stride, const float* anchors, int B,
                       int num_classes, float score_thr, float iou_thr, int max_per_class, float img_w, float img_h,
                       const float* stds, float* out, int* counts, void* stream);

/* MultiBox training loss of the SSD detector and its gradients with respect to the head outputs (csrc/ssd_loss.hip; the
 * training half of configs/detection/mnv2_ssd_300_2_heads.py:41-55: MaxIoUAssigner(pos_iou_thr = neg_iou_thr = 0.4,
 * min_pos_iou = 0, gt_max_assign_all = False), smoothl1_beta = 1, neg_pos_ratio = 3), two launches, nothing read back.
 * Arithmetic per the published mmdet 2.x SSDHead.loss / MaxIoUAssigner / DeltaXYWHBBoxCoder / smooth_l1_loss, restated in
 * tests/ssd_loss_ref.py; parity with the reference's detector is unpinned (the fork is external); the config's
 * loss_balancing has no published definition and is not built.
 *   dtype .. reg_stride, anchors: as t3d_ssd_decode_nms (pad channels are never read); A = sum hw*nanchors;
 *   gt_boxes [B][G][4] fp32 (x1, y1, x2, y2 in input pixels), gt_labels [B][G] int32, gt_counts [B] int32 clamped to
 *   [0, G]; a slot below the count is used when its coordinates are finite, x2 > x1, y2 > y1 and 0 <= label < num_classes,
 *   and skipped as if absent otherwise.
 * Per image: IoU in fp32, every operation rounded on its own; assigned[a] = the first ground truth of the largest IoU when
 * that is >= pos_iou_thr, else -1; then, ground truths ascending, the LOWEST anchor of the largest IoU is given to the ground
 * truth when that IoU >= min_pos_iou (a later one overrides; with min_pos_iou = 0 a ground truth that overlaps nothing takes
 * anchor 0); positives carry gt_labels[assigned], all others the background class num_classes; ce in fp32 (expf / logf);
 * the k = min(neg_pos_ratio * num_pos, num_neg) negatives first by (ce descending on the fp32 bit pattern, anchor ascending)
 * are mined; box targets ((gx-px)/pw, (gy-py)/ph, log(gw/pw), log(gh/ph)) / stds, smooth L1 with beta.
 * Over the batch, avg = max(sum num_pos, 1):
 *   scalars [4] fp64 = loss_cls (ce of positives and mined negatives / avg), loss_bbox (/ avg), total_pos, total_mined;
 *   sums in fp64 over a fixed tree (no floating-point atomics: two runs are bit-identical);
 *   num_pos [B] int32; assigned [B][A] int32: ground-truth index, -1 unused negative, -2 mined negative;
 *   dcls / dreg: HOST arrays of nlevels fp32 device pointers in the rows and strides of cls / reg:
 *   dcls = (softmax - onehot(label)) / avg on positives and mined negatives, dreg = smoothl1'(reg - t) / avg on positives,
 *   0 elsewhere, pad channels included; both NULL = losses only.
 *   work: t3d_ssd_multibox_work_bytes(B, A) bytes of device scratch, 8-byte aligned (RETURNS the byte count, or T3D_ERR_ARG).
 * T3D_ERR_ARG: NULL or misaligned arguments, G < 0, nlevels outside 1..2, only one of dcls / dreg, beta <= 0,
 * neg_pos_ratio < 0, work_bytes too small.  T3D_ERR_UNSUPPORTED: neg_iou_thr != pos_iou_thr (no ignore band), A > 16384 or
 * G > 64 (the per-anchor state of an image lives in LDS), B * A >= 2^31.  B == 0 returns T3D_OK without a launch. */
int t3d_ssd_multibox_work_bytes(int B, int A);
int t3d_ssd_multibox_loss(int dtype, int nlevels, const void* const* cls, const void* const* reg, const int* hw,
                          const int* nanchors, const int* cls_stride, const int* reg_stride, const float* anchors,
                          const float* gt_boxes, const int* gt_labels, const int* gt_counts, int B, int G, int num_classes,
                          float pos_iou_thr, float neg_iou_thr, float min_pos_iou, int neg_pos_ratio, float beta,
                          const float* stds, void* work, long long work_bytes, double* scalars, int* num_pos, int* assigned,
                          void* const* dcls, void* const* dreg, void* stream);

/* Backward of the SSD heads' second half, ReLU(BatchNorm(y)) -> 1x1 conv + bias (csrc/ssd_head_bwd.hip): what training the
 * SSDHead of configs/detection/mnv2_ssd_300_2_heads.py:15-37 under its optimizer / lr_config :145-153 needs between the
 * MultiBox loss above and the depthwise layers, for EVERY head in one call of two launches (the pass, the ordered finish).
 * Per head i (all arrays are HOST arrays of length nheads, device pointers in the pointer arrays):
 *   dout  [M][ns] fp32: the loss's gradient at the head's output as t3d_ssd_multibox_loss wrote it (pad columns n..ns-1 are 0
 *         by that contract; they are read and multiplied by zero, so they must be finite); never rounded to the storage dtype;
 *   y     [M][C] (dtype): the raw depthwise output; scale, shift [C] fp32 and `act` (T3D_ACT_RELU, or T3D_ACT_NONE): the
 *         prologue the forward 1x1 conv applied on load;  w [ns][C] (dtype): the matrix that conv multiplied by (rows past n
 *         are not read);
 *   g     [M][C] (dtype) = (dout . W) where fmaf(y, scale, shift) > 0 -- the forward's own comparison --, else 0: the gradient
 *         at the BatchNorm output; the dot product runs in fp64, g is rounded once on store;
 *   stats [2C] fp64 += sum(g), sum(g*y) of the unrounded g (what t3d_bn_bwd_finalize reads; the caller zeroes it);
 *   dW    [n][C] fp32 = dout^T relu(fmaf(y, scale, shift)), OVERWRITTEN;  dbias [n] fp32 = column sums of dout, OVERWRITTEN.
 * Sums over M: fp32 inside a workgroup's 128 rows (dW) or fp64 (the others), fp64 across workgroups, in a fixed order -- no
 * floating-point atomics, two runs are bit-identical.
 *   work: t3d_ssd_head_bwd_work_bytes(nheads, M, C, n) bytes of device scratch, 16-byte aligned (the query RETURNS the byte
 *   count, or a negative T3D_ERR_*).
 * T3D_ERR_UNSUPPORTED: C % 8 != 0, C > 1024, ns > 64, ns % 8 != 0, more than 8 heads, T3D_F16, another activation.
 * T3D_ERR_ARG: n < 1, n > ns, M < 0, an unknown dtype, NULL or misaligned pointers (dout: 16 bytes), work_bytes too small.
 * Every check precedes the first launch.  nheads == 0, or M == 0 for every head, launches nothing and returns T3D_OK; a head
 * with M == 0 beside others gets dW = dbias = 0. */
int t3d_ssd_head_bwd_work_bytes(int nheads, const int* M, const int* C, const int* n);
int t3d_ssd_head_bwd(int dtype, int nheads, const void* const* dout, const void* const* y, const void* const* scale,
                     const void* const* shift, const void* const* w, const int* M, const int* C, const int* n, const int* ns,
                     int act, void* const* g, void* const* stats, void* const* dW, void* const* dbias, void* work,
                     long long work_bytes, void* stream);

/* The demo's third stage: IOUTracker.process + get_tracked_objects of torchdet3d/utils/tracking_tools.py:127-290 (Track:
 * :9-124; call site scripts/demo.py:56-78), one frame of S independent streams (cameras) per launch, one workgroup per
 * stream; the whole tracker state lives in device memory and nothing is read back.  Per stream, in the reference's order:
 * active tracks (end_time >= time - continue_time_thresh) in list order; cost[i][j] = 0.5 (1 - GIoU(det_i, last_box_j)) in
 * fp64, stored as fp32; a minimum-cost assignment of the rectangular matrix (shortest augmenting paths with potentials, fp64
 * on the fp32 costs; among equal optima which one is returned is unspecified); a pair survives when cost < match_threshold
 * and IoU(last_box, det) > track_detection_iou_thresh; Track.add_detection (interpolation over a gap 1 < skip <=
 * continue_time_thresh, box EMA int((1 - s) prev + s new) in fp64, the three-branch keypoint filter and the optional align_kp
 * swap search); one new track per unassigned detection in detection order (id: FIFO of released ids, else last_global_id++);
 * _clear_old_tracks with a stable compaction; then the get_tracked_objects selection at the advanced time.
 * Deviations: only the LAST box / keypoints and the length of a track are kept (no histories, no archive: `cleared` counts
 * the tracks that left through track_clear_thresh); keypoints are fp64 throughout; the table holds max_tracks tracks -- a
 * detection that would open a track in a full table is not tracked and `dropped` is incremented.
 *   state  [S][t3d_track_state_bytes(max_tracks)] bytes; ALL ZERO = a fresh tracker (time 0, no tracks, no ids handed out);
 *   dets   [S][max_dets][4] int32 (left, top, right, bottom);  kps [S][max_dets][18] fp32;
 *   counts [S] int32 valid detections per stream, clamped to [0, max_dets]; NULL: max_dets for every stream;
 *   the eleven arguments of IOUTracker.__init__ (interpolate_time_thresh is stored but never read by the reference);
 *   out_count [S]; out_boxes [S][max_tracks][4] int32; out_kp [S][max_tracks][18] fp64; out_ids [S][max_tracks] int32, -1 for a
 *   track not longer than time_window (label 'ID -1'); rows past out_count are left as they were;
 *   out_scalars [S][4] int32 = num_tracks, last_global_id, time, dropped.
 * T3D_ERR_UNSUPPORTED when t3d_track_lds_bytes(max_dets, max_tracks) exceeds the 160 KiB of LDS a workgroup can have.
 * t3d_track_state_bytes / t3d_track_lds_bytes RETURN byte counts (or T3D_ERR_ARG). */
int t3d_track_state_bytes(int max_tracks);
int t3d_track_lds_bytes(int max_dets, int max_tracks);
int t3d_track_step(void* state, const int* dets, const float* kps, const int* counts, int S, int max_dets, int max_tracks,
                   int time_window, int continue_time_thresh, int track_clear_thresh, double match_threshold,
                   double track_detection_iou_thresh, int interpolate_time_thresh, double detection_filter_speed,
                   double keypoints_filter_speed, double add_treshold, int no_updated_frames_treshold, int align_kp,
                   int* out_count, int* out_boxes, double* out_kp, int* out_ids, int* out_scalars, void* stream);

/* The joints of the live pipeline (scripts/demo.py:56-78: detector -> regressor -> tracker -> keypoints in frame pixels) on
 * the device (csrc/pipeline.hip), so that a frame is one chain of launches with no host round trip.
 *
 * t3d_ssd_select_rects: t3d_ssd_decode_nms's out [F][num_classes][max_per_class][6] / counts [F][num_classes] -> per frame
 * the list the host code builds today (models/ssd.py: SSD300.detect's merge, utils/ie_wrappers.py:94-120:
 * Detector._decode_detections), cut to max_dets rows; one workgroup per frame, every step in the host's own precision:
 *   the rows class-major, the first counts[f][c] of each class; stable sort by descending score, the first max_per_img;
 *   x / input_size in fp32; a row stays when score > conf (fp32: a score equal to the rounded threshold is dropped);
 *   left = (int)((x1 > 0 ? x1 : 0) * (float)frame_w), an fp32 product truncated towards zero; top / right / bottom alike;
 *   unless (expand_w, expand_h) == (1, 1): w = right - left, dw = w * (expand_w - 1) / 2 in fp64,
 *   left = max((int)(left - dw), 0), right = (int)(right + dw); top / bottom alike with expand_h;
 *   stable sort by descending top; the first max_dets.
 *   rects [F][max_dets][4] int32 (left, top, right, bottom: the unclipped frame-pixel boxes);
 *   crop_rects [F*max_dets][4] int32: the same boxes clamped to [0, frame_w] x [0, frame_h] (numpy slice semantics) with
 *   f * frame_h added to the rows -- rectangles into the F frames stacked as ONE frame of F * frame_h rows, which is how
 *   t3d_crop_resize_u8 crops all of them in one launch;
 *   scores [F][max_dets] fp32; det_labels [F][max_dets] int32; counts [F] int32 rows written (<= max_dets);
 *   overflow [F] int32: rows that passed the threshold and fell to the cap max_dets.
 * Rows at or past counts[f] are ZERO in every output (t3d_crop_resize_u8 makes black crops of them).
 * T3D_ERR_UNSUPPORTED when num_classes * max_per_class > 4096 (the candidates of a frame are sorted in LDS). */
int t3d_ssd_select_rects(const float* out, const int* cnt, int F, int num_classes, int max_per_class, int max_per_img,
                         float input_size, float conf, int frame_h, int frame_w, double expand_w, double expand_h,
                         int max_dets, int* rects, int* crop_rects, float* scores, int* det_labels, int* counts, int* overflow,
                         void* stream);

/* The head of the arg-max class (utils/ie_wrappers.py:135-139): kp_all [num_heads][n][18] fp32 (t3d_head_fwd_all), logits
 * [n][num_classes] fp32 -> labels [n] int32 = the lowest index among the row's maxima (0 when num_classes <= 1 or logits is
 * NULL), kp [n][18] = kp_all[labels[i]][i].  One workgroup per row.  num_classes <= num_heads. */
int t3d_head_select(const float* kp_all, const float* logits, int n, int num_heads, int num_classes, int* labels, float* kp,
                    void* stream);

/* Regressor.transform_kp (utils/ie_wrappers.py:144-152) on every tracked object (scripts/demo.py:78), one workgroup per
 * stream, from t3d_track_step's outputs: kp_frame [S][max_tracks][18] fp64, x = round(kp_x * (right - left)) then
 * round(x + left), y alike with top / bottom -- two fp64 roundings, as numpy does them.  Rows past out_count[s] are left
 * as they were. */
int t3d_track_kp_to_frame(const int* out_count, const int* out_boxes, const double* out_kp, double* kp_frame, int S,
                          int max_tracks, void* stream);

/* The last stage of the live loop (scripts/demo.py:26-46 draw_detections + utils/utils.py:247-270 draw_kp): rectangles, the
 * 12 box edges, 9 keypoint discs and a label plate with text, drawn IN PLACE on frames [S][H][W][3] uint8 by one launch for
 * all cameras (csrc/draw.hip).  OpenCV and objectron.graphics are absent, so the raster rules are this project's own, all in
 * integers (DESIGN.md section 7 states them; tests/draw_ref.py restates them in numpy and the kernel is bit-equal to that);
 * the LOOK (colours, thickness, font) is unpinned against the reference's output.
 *   count [S] int32 or NULL (= T objects per camera), clamped to [0, T]; objects are drawn in index order, a later object
 *   over an earlier one; within an object: rectangle (boxes [S][T][4] int32 left, top, right, bottom, or NULL: none), the
 *   12 edges (4 along x, 4 along y, 4 along z, a colour per axis), discs of keypoints 0..8, label plate, label text.
 *   kp [S][T][18] fp64 in frame pixels (FramePipeline's kp_frame); a point is rint(x), rint(y) (half to even) and is skipped,
 *   with every edge that uses it, unless both are finite and |.| <= 8191.
 *   ids [S][T] int32 or NULL; ids < 0 (the tracker's "not longer than time_window"): the rectangle takes the "off" colour,
 *   edges and discs are not drawn, plate and text are.
 *   labels: object t of camera s has class labels[s * label_stride + t] when t < label_count[s] (clamped to
 *   [0, label_stride]; NULL label_count: every entry), else none; the text is the Objectron class name of a label in 0..8,
 *   followed by " <id>" when flags has T3D_DRAW_IDS and id >= 0; an empty text has no plate.  NULL labels: no class text.
 * style is a HOST struct, copied into the launch: rect_th, edge_th in 1..16, kp_radius in 0..32, font_scale in 1..8 (the
 * font is a 5 x 7 bitmap, a font pixel is font_scale x font_scale, the advance 6 * font_scale), colours in the frame's own
 * channel order: rectangle, rectangle "off", edges along x / y / z, keypoint, plate, text.
 * 1 <= H, W <= 8192, 1 <= T <= 1024, S <= 65535; S == 0 returns T3D_OK without a launch; T3D_ERR_ARG for NULL frames / kp /
 * style, sizes or style fields out of range, label_stride < 1 (or < T with a NULL label_count) when labels is given.
 * A workgroup owns a 64 x 16 pixel tile and leaves without touching global memory when no primitive's bounding box meets
 * it; a thread stores only bytes of its own four pixels (aligned dwords when frames is 4-byte aligned and W % 4 == 0, bytes
 * otherwise); no global atomics: the result does not depend on scheduling.
 * t3d_draw_glyphs copies the font out: 38 glyphs (a-z, 0-9, '_', ' ') of 7 row bytes, column c of a row at bit 4 - c; any
 * other character is drawn as a filled cell.  Copies min(bytes, 266) bytes and RETURNS 266 (T3D_ERR_ARG: bytes < 0, or a
 * NULL out with bytes > 0). */
#define T3D_DRAW_IDS 1
typedef struct {
  int rect_th, edge_th, kp_radius, font_scale, flags;
  unsigned char colors[8][3];
} t3d_draw_style;
int t3d_draw_overlays_u8(unsigned char* frames, int S, int H, int W, const int* count, const int* boxes, const double* kp,
                         const int* ids, const int* labels, const int* label_count, int label_stride, int T,
                         const t3d_draw_style* style, void* stream);
int t3d_draw_glyphs(unsigned char* out, int bytes);

/* The Objectron evaluation protocol of the reference's final report (scripts/objectron_eval.py:116-175 around
 * objectron.dataset.eval.Evaluator) on the device (csrc/objectron_eval.hip), F frames per launch pair, fp64 throughout.
 * The dependency is absent from the reference: DESIGN.md section 7 states the protocol, parity with
 * the upstream package is unpinned.
 *
 * t3d_objectron_pairs: one workgroup per (frame, prediction slot): match, lift, ground-plane scale, the six metrics.
 *   pred_kp [F][P][9][2] fp64 keypoints, multiplied by (sx, sy) on load: (1, 1) for keypoints normalised to the frame,
 *   (1 / W, 1 / H) for frame pixels (FramePipeline's kp_frame [S][T][18]);  pred_count [F] int32, clamped to [0, P];
 *   gt_kp2d [F][G][9][2] fp64 normalised; gt_kp3d [F][G][9][3] fp64, camera frame, metric scale; gt_visibility [F][G] fp64;
 *   gt_count [F] int32, clamped to [0, G]; planes [F][6] fp64 = centre, normal.
 *   A prediction matches i* = argmin_i ||pred[1:9] - kp2d_i[1:9]||_F (first minimum), or nothing when visibility[i*] < 0.1.
 *   metrics [F][P][6] fp64 = pixel, azimuth, polar, iou, add, adds -- unmatched: 0.1, 30, 20, 0, 1, 1; matched: mean corner
 *   pixel distance; lift_2d(pred, portrait) with the default NDC camera, scaled by mean(centre.normal / d[0:4]), d = the
 *   ascending corner dot products with the normal; absolute azimuth (wrapped at 180) / polar difference in degrees of the
 *   viewpoints (T = Oh Vh^T (Vh Vh^T)^-1 with O the unit box scaled by V's edge lengths; (x, y, z) = T[0:3][3]); the IoU of
 *   t3d_box_iou3d; mean corner distance and mean nearest-corner distance over the 9 vertices.  A non-finite intermediate is
 *   carried into the metric (no trap).  matched [F][P] int32 = i* or -1.  Slots at or past pred_count[f] are left untouched.
 *
 * t3d_objectron_hitmiss: one workgroup per frame, writes row base + f of the evaluator's record (capacity rows):
 *   valid [row] = 1 when the frame has an instance with visibility > 0.1, centre keypoint strictly inside (0, 1)^2 and
 *   kp3d[0].z < 0, else 0 and the rest of the row is zero; num_instances [row] = the clamped gt_count[f];
 *   thresholds [6][21] fp64 in the metric order above (computed by the HOST: numpy.linspace, never on the device);
 *   hit / miss [row][6][21] int32 over the frame's predictions in slot order: hit when iou >= thr, or value <= thr for the
 *   other five (a nan misses everywhere);  sums [row][5] fp64 = error_2d, iou_3d, azimuth, polar over the matched
 *   predictions (finite values only), matched count.  Deterministic: plain stores, no atomics.
 * Both only enqueue on `stream`; T3D_ERR_ARG for a NULL pointer, F, P or G <= 0, base < 0 or base + F > capacity. */
int t3d_objectron_pairs(const double* pred_kp, const int* pred_count, const double* gt_kp2d, const double* gt_kp3d,
                        const double* gt_visibility, const int* gt_count, const double* planes, int F, int P, int G, double sx,
                        double sy, double* metrics, int* matched, void* stream);
int t3d_objectron_hitmiss(const double* metrics, const int* matched, const int* pred_count, const double* gt_kp2d,
                          const double* gt_kp3d, const double* gt_visibility, const int* gt_count, const double* thresholds,
                          int F, int P, int G, int base, int capacity, int* valid, int* num_instances, int* hit, int* miss,
                          double* sums, void* stream);

/* COCO bbox evaluation of the detector on the device (csrc/detection_eval.hip): the per-image half of the published
 * pycocotools COCOeval with iouType = 'bbox', as mmdet 2.x's CocoDataset.evaluate(metric='bbox') drives it for
 * configs/detection/mnv2_ssd_300_2_heads.py:56-60,130-143.  pycocotools is not installed where this project is built:
 * DESIGN.md section 7 states the protocol, tests/coco_eval_ref.py restates it as loops, parity with the package is unpinned.
 * Deviations: no crowd branch (annotation_converters/objectron_2_coco.py:170 writes iscrowd = 0 everywhere), NMS at input
 * scale before the rescale where mmdet rescales first, no xywh round trip through JSON.
 *
 * t3d_ssd_cap_per_image: mmdet's test_cfg.max_per_img on the device, one workgroup per image.
 *   out [B][num_classes][max_per_class][6] fp32 / counts [B][num_classes] int32 as t3d_ssd_decode_nms leaves them (counts
 *   clamped to [0, max_per_class]; only column 4, the score, of the rows below a count is read; `out` is never written).
 *   Of all valid rows of an image the first max_per_img survive in the order score descending (a nan last), then class
 *   ascending, then row ascending -- numpy's stable argsort of -score over the classes' rows concatenated, which is what
 *   SSD300.merge_classes does on the host.  counts_out [B][num_classes] int32 = the survivors of each class; with the rows of
 *   a class in non-increasing score order (the decode kernel's greedy NMS emits them so) they are the class's first
 *   counts_out rows.  counts_out may be `counts` itself.
 *   T3D_ERR_ARG: NULL or misaligned pointers, B < 0, num_classes < 1, max_per_class < 1, max_per_img < 0.
 *   T3D_ERR_UNSUPPORTED: num_classes * max_per_class > 4096 (an image's scores are ranked in LDS).  B == 0: T3D_OK, no launch.
 *
 * t3d_coco_match: COCOeval.evaluateImg for every (image, class) of a batch, one workgroup per cell, into rows
 * base .. base + B - 1 of a record of R rows.
 *   out / counts as above (counts already capped); gt_boxes [B][G][4] fp32 (x1, y1, x2, y2 in input pixels), gt_labels
 *   [B][G] int32, gt_counts [B] int32 clamped to [0, G]: a slot below the count is used when its coordinates are finite,
 *   x2 > x1, y2 > y1 and 0 <= label < num_classes, and skipped as if absent otherwise (the rule of t3d_ssd_multibox_loss);
 *   both may be NULL when G == 0.  ori_shapes [B][2] int32 = (h, w) of the original frame, (in_w, in_h) the network input;
 *   iou_thrs [10] fp64, area_rngs [4][2] fp64 (lo, hi), both computed by the HOST (numpy.linspace; never on the device).
 *   Coordinates: fx = (double)w / (double)in_w, fy = (double)h / (double)in_h, X = (double)x * fx, Y = (double)y * fy,
 *   area = (X2 - X1) * (Y2 - Y1); fp64 from there on, every operation rounded on its own.
 *   Detections of a cell: its first min(counts, 100) rows, taken to be in non-increasing score order.
 *   IoU(d, g): iw = min(dX2, gX2) - max(dX1, gX1), ih likewise; 0 when iw <= 0 or ih <= 0, else i = iw * ih,
 *   i / (ad + ag - i).
 *   Per area range a and threshold t: a ground truth is ignored when ag < lo[a] or ag > hi[a]; ground truths are walked
 *   non-ignored first, then ignored, each group in slot order; per detection thr = min(T[t], 1 - 1e-10), m = none; a ground
 *   truth already matched at (a, t) is skipped; the walk STOPS when m is set, m is not ignored and this one is; one with
 *   iou < thr is skipped; otherwise thr = iou, m = this one (equality matches: among equal IoUs the later wins).  A matched
 *   detection gets dtm = 1, dtig = ignored(m), and m is taken; an unmatched one dtig = (ad < lo[a] or ad > hi[a]).
 *   Record row r = base + b, every slot written (nothing needs clearing):
 *     rec_score [R][num_classes][100] fp32 (0 past the cell's detections);
 *     rec_dtm / rec_dtig [R][num_classes][100] uint64, bit a * 10 + t (0 past the cell's detections);
 *     rec_ndt [R][num_classes] int32; rec_ngt [R][num_classes][4] int32 = non-ignored ground truths per area range;
 *     rec_valid [R] int32 = 1, or 0 for a frame with h <= 0 or w <= 0, whose row is then empty.
 *   T3D_ERR_UNSUPPORTED: G > 64 (the IoU matrix of a cell lives in LDS; the loss kernel's bound).
 *   T3D_ERR_ARG: NULL or misaligned pointers (8 bytes for the fp64 / uint64 ones), B, G, base or R < 0, base + B > R,
 *   num_classes < 1, max_per_class < 1, in_w <= 0 or in_h <= 0.  B == 0 returns T3D_OK without a launch.  Every check
 *   precedes the launch.  No atomics: each cell has one owner, two runs are bit-identical.  Both only enqueue on `stream`. */
int t3d_ssd_cap_per_image(const float* out, const int* counts, int B, int num_classes, int max_per_class, int max_per_img,
                          int* counts_out, void* stream);
int t3d_coco_match(const float* out, const int* counts, int B, int num_classes, int max_per_class, const float* gt_boxes,
                   const int* gt_labels, const int* gt_counts, int G, const int* ori_shapes, int in_w, int in_h,
                   const double* iou_thrs, const double* area_rngs, int base, int R, float* rec_score,
                   unsigned long long* rec_dtm, unsigned long long* rec_dtig, int* rec_ndt, int* rec_ngt, int* rec_valid,
                   void* stream);

/* ---- ResNet-50 backbone (BASELINE config 4; the reference has no ResNet -- standard torchvision architecture, parity
 * against oracle/resnet.py, unpinned).  Dense k x k convolutions run as patch gather + the pointwise GEMM entry points
 * (t3d_pwconv_fwd / _dgrad / _wgrad with K = Kp); everything below is an HBM-bound gather / elementwise kernel. ---- */

/* nn.Conv2d(C, N, k, stride, pad) input side: x [B,H,W,C] raw tensor read through `pro` (BatchNorm affine + activation of
 * its producer; NULL: finished tensor), zero padding applied to the ACTIVATED tensor -> col [B*Ho*Wo][Kp],
 * column (ky*k + kx)*C + c, columns k*k*C .. Kp-1 zero (Kp: multiple of 8).  _nchw: the fp32 NCHW crops of the input
 * contract (stem). */
int t3d_im2col(int dtype, const void* x, const t3d_prologue* pro, void* col, int B, int H, int W, int C, int k, int stride,
               int pad, int Kp, void* stream);
int t3d_im2col_nchw(int dtype, const float* x, void* col, int B, int H, int W, int C, int k, int stride, int pad, int Kp,
                    void* stream);
/* Backward of t3d_im2col: dcol [B*Ho*Wo][Kp] (= dy W, from t3d_pwconv_dgrad) -> dx [B,H,W,C] = gradient at the producer's
 * BatchNorm output (patch gradients summed per input pixel, times act'(scale*x_raw + shift)); stats [2*C] fp64 or NULL:
 * += sum(dx), sum(dx * x_raw) (replicas as elsewhere). */
int t3d_col2im_bwd(int dtype, const void* dcol, const void* x_raw, const t3d_prologue* pro, void* dx, double* stats, int B,
                   int H, int W, int C, int k, int stride, int pad, int Kp, void* stream);
/* [N][C][k][k] fp32 master weight -> [N][Kp] GEMM operand in patch-column order (storage dtype), and the gradient back. */
int t3d_pack_conv_weight(int dtype, const float* w, void* out, int N, int C, int k, int Kp, void* stream);
int t3d_unpack_conv_grad(const float* dw_packed, float* dw, int N, int C, int k, int Kp, void* stream);
/* nn.MaxPool2d(3, 2, 1) over act(scale*y + shift): out [B,Ho,Wo,C] finished tensor, argmax [B,Ho,Wo,C] uint8 (window
 * position 0..8, first maximum in scan order); backward: dy = gradient at y's BatchNorm output + its backward sums. */
int t3d_maxpool_fwd(int dtype, const void* y, const t3d_prologue* pro, void* out, unsigned char* argmax, int B, int H, int W,
                    int C, void* stream);
int t3d_maxpool_bwd(int dtype, const void* dout, const unsigned char* argmax, const void* y, const t3d_prologue* pro, void* dy,
                    double* stats, int B, int H, int W, int C, void* stream);
/* Bottleneck tail  z = relu(BN3(y3) + shortcut):  shortcut read through pro_s (projection shortcut: raw 1x1 output +
 * its BatchNorm) or as it is (identity, pro_s NULL).  Backward: g = dz * [z > 0] (the gradient at BOTH BatchNorm
 * outputs); stats3 += sum g, sum g*y3; statsd (with yd) += sum g, sum g*yd. */
int t3d_res_relu_fwd(int dtype, const void* y3, const t3d_prologue* pro3, const void* shortcut, const t3d_prologue* pro_s,
                     void* z, int M, int C, void* stream);
int t3d_res_relu_bwd(int dtype, const void* dz, const void* z, const void* y3, const void* yd, void* g, double* stats3,
                     double* statsd, int M, int C, void* stream);
/* upsample == 0: out [B,Ho,Wo,C] = x[:, ::stride, ::stride, :] (x [B,H,W,C]);  upsample == 1: out [B,H,W,C] = x [B,Ho,Wo,C]
 * at the multiples of stride, zero elsewhere (gradient of the former). */
int t3d_subsample(int dtype, const void* x, void* out, int B, int H, int W, int C, int stride, int upsample, void* stream);

/* Reduction replicas.  Every `+=` reduction output of the kernels (the fp64 BatchNorm sums `stats`, the depthwise
 * weight gradient `dw`) is hit by one atomic per channel per workgroup; with hundreds of workgroups on a few KB of
 * addresses those atomics serialise.  With nrep > 1 the streaming kernels add into replica (workgroup % nrep):
 *   stats replica r lives at  stats + r*stats_stride  (doubles);   dw replica r at  dw + r*C*k*k  (floats);
 * t3d_bn_finalize / t3d_bn_bwd_finalize sum the nrep stats replicas, the caller sums the dw replicas.
 * Process-wide setting (default 1 = plain behaviour); kernels that do not implement replicas use replica 0. */
int t3d_set_reduction_replicas(int nrep, long long stats_stride);

/* Depthwise weight gradient without atomics (bit-reproducible).  With capacity > 0 the NEXT t3d_dwconv_bwd launches treat
 * `dw` as [capacity][C][k*k] fp32 SLOTS: every workgroup of a streaming kernel stores (does not add) its partial weight
 * gradient into its own slot and *used_out (device memory) receives the number of slots the launch filled; the caller adds
 * slots 0 .. *used_out-1 in index order (t3d_sum_slots_batched), which no longer depends on the arrival order of ~500
 * workgroups (torch's autograd makes no such promise for models/mobilenetv3.py:151 either; this is about run-to-run
 * reproducibility of the training step).  A launch that needs more workgroups than `capacity`, and the LDS-tiled fallback
 * kernel, add atomically into the first nrep slots (t3d_set_reduction_replicas) and report *used_out = nrep: those slots
 * must be zero before the launch.  capacity == 0 (default): the replica behaviour above.  Process-wide setting. */
int t3d_set_dw_slots(int capacity, int* used_out);

/* Squeeze-excite pooled sums without order noise.  on != 0: every `pooled` / `gap_sum` argument of the NEXT t3d_dwconv_fwd,
 * t3d_se_fwd_fused, t3d_se_bwd_data calls addresses int64 [B][C] in units of 2^-24 instead of float [B][C] (zero it
 * before the depthwise launch, as before): the depthwise kernel's work items add integers, which is associative, so the
 * sums -- and the gate torch computes from `y.mean((2, 3))` at models/mobilenetv3.py:100-104 -- are bit-reproducible from
 * run to run.  on == 0 (default): fp32 atomics into float [B][C].  Process-wide setting. */
int t3d_set_exact_pool(int on);

/* Measurement aid (bench.py's roofline block): attach two hipEvent_t (created with timing enabled, recorded at least once) to
 * the NEXT depthwise-convolution kernel launch -- t3d_dwconv_fwd / t3d_dwconv_bwd -- so that hipEventElapsedTime(start, stop)
 * is that kernel's own begin-to-end time (hipExtLaunchKernelGGL; what rocprofv3 --kernel-trace reports).  The pair is
 * consumed by the launch; NULL, NULL clears it. */
int t3d_set_launch_events(void* start_event, void* stop_event);
/* desc = n rows of int64 {src [slots][count] fp32, dst [count] fp32, count, used (device int*)}:
 * dst = src[0] + src[1] + ... + src[*used - 1], in that order (overwrites dst). */
int t3d_sum_slots_batched(const long long* desc, int n, void* stream);

/* BatchNorm finalize derived by the CONSUMER.  t3d_bn_finalize / t3d_bn_bwd_finalize are 5-us launches that sit
 * between every convolution and its consumer (~100 per training step, all on the critical stream: 0.64 ms of an
 * 8.4-ms MobileNetV2 step with the launch gaps).  A fold request names a coefficient array (`key`: the `scale` pointer
 * of a t3d_prologue, or the `alpha` pointer of a t3d_bnbwd) and a DEVICE-resident descriptor of everything the finalize
 * would compute; the NEXT launch that takes exactly that array as its prologue / BatchNorm-backward coefficients
 * consumes the request: its workgroups derive the coefficients of their own channels from the replica sums (the
 * kernel boundary already orders the sums before them -- no device-wide barrier), and one workgroup per channel also
 * writes the finalize's outputs for every later reader.  Implemented by the bf16 streaming kernels (t3d_pwconv_fwd /
 * _dgrad / _wgrad (the weight gradient derives without publishing), t3d_dwconv_fwd / _bwd with k = 3) and
 * t3d_bn_apply, t3d_se_bwd_affine (round 6); other launches
 * leave the request pending: check t3d_fold_pending() (returns 1 and clears it) right after the launch -- the launch
 * then read unfinalized coefficients and must be treated as failed (the entry points listed above fall back to a
 * finalize launch of their own on code paths without the derive prologue, e.g. fp32 storage).
 *   kind 1 (forward, = t3d_bn_finalize):      stats = sum(y), sum(y^2); o0..o3 = scale, shift, mean, invstd
 *   kind 2 (backward, = t3d_bn_bwd_finalize): stats = sum(dz), sum(dz*y); o0..o4 = alpha, beta, gammac, dgamma, dbeta */
typedef struct {
  int kind;
  int C;
  int nrep;                  /* reduction replicas behind `stats` ... */
  long long rstride;         /* ... replica r at stats + r*rstride (doubles) */
  const double* stats;
  double count;
  const float *gamma, *beta;
  float *rm, *rv;            /* kind 1: running estimates (may be NULL) */
  long long* nbt;            /* kind 1: num_batches_tracked (may be NULL) */
  float momentum, eps;
  float *o0, *o1, *o2, *o3, *o4;
  const float *mean, *invstd; /* kind 2: the forward's batch mean / invstd */
} t3d_bn_fold;
int t3d_fold_request(const t3d_bn_fold* desc_device, const void* key);
int t3d_fold_pending(void);

/* Optional device scratch (caller-owned, process-wide setting; NULL/0 clears it).  With a workspace the bf16
 * pointwise weight gradient writes its per-split partial dW tiles there with plain stores and reduces them in a
 * second, deterministic pass; without one the partials leave as fp32 atomics.  64 MB covers every layer shape of
 * the supported models at batch 256. */
int t3d_set_workspace(void* ptr, long long bytes);
/* Scratch for launches on the caller's MAIN stream (the workspace above belongs to the weight-gradient launches, which the
 * host side issues on a second stream): the fp32 pointwise kernel splits the contraction of few-pixel, deep layers over it
 * (classifier Linear(960, 1280) on 256 samples: 16 workgroups x 40 serial rounds otherwise).  NULL / 0 = unsplit. */
int t3d_set_main_workspace(void* ptr, long long bytes);

/* All weight matrices of a model in ONE launch: desc is a DEVICE array of n records of 7 int64
 * {src fp32 [rows,cols], out [rows,cols] or 0, out_t [cols,rows] or 0, rows, cols, frag or 0, frag_t or 0} (outputs in `dtype`);
 * frag / frag_t: fragment-order copies of the matrix / of its transpose (t3d_pwconv_pack_frag; t3d_pwconv_frag_bytes(rows, cols)
 * / (cols, rows) bytes, cleared once by the caller: only the elements of the matrix are written). */
int t3d_pack_weights_batched(int dtype, const long long* desc, int n, void* stream);

/* Optimizer step: torch.optim.AdamW as build_optimizer(name='adam') constructs it
 * (torchdet3d/builders/optim_builder.py:10-12; stepped at trainer/train.py:50-52) over ONE flat fp32 buffer of n
 * elements (n % 4 == 0): decoupled weight decay, no amsgrad.  `step` is the 1-based step count (bias corrections are
 * computed on the host in fp64), g is read as grad_scale * g (1/world for summed data-parallel gradients), m / v are the
 * caller-owned moment buffers (zeroed before the first step). */
int t3d_adamw_step(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2,
                   double eps, double weight_decay, long long step, double grad_scale, void* stream);
/* The other three names of build_optimizer (torchdet3d/builders/optim_builder.py:3-19), same contract as t3d_adamw_step: ONE
 * launch over the flat fp32 buffer (n % 4 == 0), g read as grad_scale * g, state buffers caller-owned and zeroed before the
 * first step, `step` the 1-based step count (what the divergence watch below reports), `lr` and `step` at fixed positions so
 * that a step plan binds them to slots.  The arithmetic is torch.optim's single-tensor path with coupled weight decay
 * g' = g + weight_decay * p; derived constants (1 - alpha, 1 - rho) are formed on the host in fp64.
 *  _sgd_step      torch.optim.SGD(lr, momentum, weight_decay, nesterov) (optim_builder.py:15-17): buf = momentum*buf + g';
 *                 d = g' + momentum*buf (nesterov) or buf; p -= lr*d.  Dampening 0.  momentum == 0: buf may be NULL, d = g'
 *                 (nesterov != 0 is then an argument error, as in torch);
 *  _rmsprop_step  torch.optim.RMSprop(lr, alpha, weight_decay) (optim_builder.py:13-14), not centered, no momentum:
 *                 sq = alpha*sq + (1-alpha)*g'^2; p -= lr * g' / (sqrt(sq) + eps);
 *  _adadelta_step torch.optim.Adadelta(lr, rho, weight_decay) (optim_builder.py:7-9): sq = rho*sq + (1-rho)*g'^2;
 *                 delta = sqrt(acc + eps) / sqrt(sq + eps) * g'; acc = rho*acc + (1-rho)*delta^2; p -= lr*delta.
 * All three are stepped where the reference steps its optimizer, trainer/train.py:50-52. */
int t3d_sgd_step(float* p, const float* g, float* buf, long long n, double lr, double momentum, double weight_decay,
                 int nesterov, long long step, double grad_scale, void* stream);
int t3d_rmsprop_step(float* p, const float* g, float* sq, long long n, double lr, double alpha, double eps,
                     double weight_decay, long long step, double grad_scale, void* stream);
int t3d_adadelta_step(float* p, const float* g, float* sq, float* acc, long long n, double lr, double rho, double eps,
                      double weight_decay, long long step, double grad_scale, void* stream);
/* Divergence watch for the optimizer steps that follow (process-wide, like t3d_set_reduction_replicas): with a DEVICE
 * int64 word set (the caller initialises it to INT64_MAX), every optimizer step of this header (t3d_adamw_step, t3d_sgd_step,
 * t3d_rmsprop_step, t3d_adadelta_step) does *word = min(*word, step) when it meets a non-finite gradient element; NULL
 * switches it off.  Serves the loss the reference's loop reads at train.py:57 -- after a
 * divergence `loss.item()` is NaN there, while the clamp-form ReLU6 of the 16-bit kernels can leave this path's loss
 * finite: the trainer reports NaN from the first watched step on, per step and identically on every rank (the gradient is
 * all-reduced before the optimizer reads it). */
int t3d_set_grad_watch(long long* first_bad_step);

/* Small bookkeeping kernels that keep the step free of framework arithmetic:
 *  _copy_cols   dst [rows,cols_dst] <- leading columns of src [rows,cols_src], rest zero (the stem's [C,27] <-> [C,32]
 *               patch-row weights and their gradient, mobilenetv3.py:110-115);
 *  _bn_bias_grad gradient of the bias of a Linear that feeds a train-mode BatchNorm1d (classifier, mobilenetv3.py:191-194):
 *               sum_b dy = alpha*sum(dz) + beta*sum(y) + count*gammac from the forward / backward sum replicas;
 *  _se_bwd_affine the per-sample BatchNorm-backward affine behind a squeeze-excite gate: aps = s*alpha, gps = gammac + g*alpha
 *               ([B,C]; what t3d_bnbwd.per_sample reads); serves a pending t3d_fold_request for `alpha` (derives AND publishes
 *               alpha / beta / gamma + the BatchNorm's parameter gradients, one owner workgroup per 32 channels);
 *  _dropout_mask nn.Dropout(p) keep/scale factors {0, 1/(1-p)} (model_builder.py:83) from Philox-4x32-10 keyed by
 *               (seed, offset): stateless and reproducible. */
int t3d_copy_cols(const float* src, float* dst, int rows, int cols_src, int cols_dst, void* stream);
int t3d_bn_bias_grad(const double* fwd_stats, const double* bwd_stats, int C, double count, const float* alpha,
                     const float* beta, const float* gammac, float* dbias, void* stream);
int t3d_se_bwd_affine(const float* s, const float* g, const float* alpha, const float* gammac, float* aps, float* gps,
                      int B, int C, void* stream);
int t3d_dropout_mask(float* mask, long long n, unsigned long long seed, unsigned long long offset, float p, void* stream);

/* Zero fill of several device buffers in one launch: desc = n rows of int64 {ptr, bytes}, bytes % 16 == 0, DEVICE array
 * (the per-step clears of the gradient buffer, the BatchNorm sum replicas and the depthwise weight-gradient replicas). */
int t3d_zero_batched(const long long* desc, int n, void* stream);

/* Fused expand 1x1 conv + BatchNorm + activation + depthwise 3x3 conv forward of an inverted-residual block (round 5;
 * csrc/expdw_fwd.hip): y2 = dwconv3x3(act(scale1 * round(W1 z) + shift1)), dtype T3D_BF16 or T3D_F16 (inference), K <= 32 (the 112x112 .. 28x28 blocks of
 * MobileNetV2), act in {T3D_ACT_RELU, T3D_ACT_RELU6}.  Replaces nn.Conv2d(K, C, 1) + nn.BatchNorm2d(C) + activation +
 * nn.Conv2d(C, C, 3, s, 1, groups=C) + the statistics pass of the following BatchNorm2d (models/mobilenetv3.py:146-153) without
 * the expanded tensor's round trip through HBM: the stencil reads it out of LDS.
 *   z [B,H,W,K] finished block input, w1 [C,K] bf16, scale1 / shift1 [C] fp32: the expansion's BatchNorm affine -- its batch
 *   statistics must exist beforehand (a statistics-only pass: t3d_pwconv_fwd / _fwd_mat with y = NULL), wdw [C,9] fp32,
 *   y1 [B,H,W,C] raw expansion or NULL (stored only for a backward that reads it), y2 [B,Ho,Wo,C] raw depthwise output,
 *   stats2 [2*C] fp64 replicas or NULL: += sum(y2), sum(y2^2) (order-independent, as t3d_dwconv_fwd).
 * T3D_ERR_UNSUPPORTED for shapes it does not take (the caller runs t3d_pwconv_fwd + t3d_dwconv_fwd);
 * t3d_expdw_supported answers that question ahead of the launch: 1 when t3d_expdw_fwd would take (dtype, act, shape), else 0
 * (an input row wider than the workgroup's fragment registers / LDS rows hold -- W > 213 -- is the case the channel tests do not
 * show: 448 ... 512-pixel inputs reach MobileNetV2's second block at W = 224 ... 256). */
int t3d_expdw_fwd(int dtype, const void* z, const void* w1, const float* scale1, const float* shift1, int act, const float* wdw,
                  void* y1, void* y2, double* stats2, int B, int H, int W, int K, int C, int stride, void* stream);
int t3d_expdw_supported(int dtype, int act, int B, int H, int W, int K, int C, int stride);

/* Step plans (round 5; csrc/plan.hip): the whole train iteration as ONE host call.
 * Replaces the per-launch host loop of torchdet3d/trainer/train.py:44-55 + builders/optim_builder.py:10-12 (model forward,
 * losses, loss.backward(), optimizer.step()): ~230 enqueue-only calls of this header that are the same from step to step
 * except for a few values.  A plan is a recorded list of
 *   calls        any enqueue entry point of this header by NAME with its arguments as 64-bit words (pointers and integers
 *                as they are, float / double as their bit patterns), the three by-pointer structs (t3d_prologue, t3d_bnbwd,
 *                t3d_loss_cfg) COPIED into the plan;
 *   forks        hipEventRecord on one stream + hipStreamWaitEvent on another (the weight-gradient stream's dependencies);
 *   read-backs   an asynchronous device-to-host copy and an event record (the step's metrics on their way to the host),
 * and t3d_plan_run replays a segment of it through the same exported entry points (same host-side state, same launches:
 * bit-identical to issuing the calls one by one).  What changes per step goes through SLOTS: an argument recorded with
 * kind 2 takes its value from slots[index] at run time (input pointers of the batch, dropout counter, optimizer step
 * count, learning rate bits, pinned read-back address, event handle).
 *   kinds[i]: 0 literal word, 1 struct (words[i] = HOST address of the struct, struct_bytes[i] its size; copied), 2 slot
 *             (words[i] = slot index);
 *   _end_segment closes the current segment and RETURNS its index (segments let a caller interleave work of its own, e.g.
 *             an RCCL all-reduce of a gradient bucket, between two runs); _num_ops RETURNS the op count (kind -1: all, 0 calls,
 *             1 forks, 2 copies, 3 event records);
 *   _time_entry switches kernel-exact event timing (t3d_set_launch_events) on / off for one entry point; _run then attaches
 *             consecutive pairs of `events` (hipEvent_t, timing enabled) to that entry point's launches in op order;
 *   _run      segment >= 0, or -1 for the whole plan; RETURNS the number of events consumed (>= 0) or T3D_ERR_*;
 *             _failed_op RETURNS the index of the op that failed (-1: none) and its return code. */
typedef struct t3d_plan t3d_plan;
int t3d_plan_create(t3d_plan** out);
int t3d_plan_destroy(t3d_plan* plan);
int t3d_plan_add_call(t3d_plan* plan, const char* entry, int nargs, const int* kinds, const unsigned long long* words,
                      const int* struct_bytes);
int t3d_plan_add_fork(t3d_plan* plan, void* from_stream, void* to_stream);
/* The fork without a packet in the producing queue: `to_stream` waits for the last kernel that call op `producer_op` (index in
 * the plan, calls / forks / copies counted alike) launches on `from_stream`, through the STOP event of that kernel's own
 * dispatch (hipExtLaunchKernelGGL) -- a device-side hand-off: the main queue of the step, whose every microsecond is on the
 * critical path, carries no event records for the ~35 launches it hands to the weight-gradient stream.
 * t3d_launch_count: how many kernels the library has launched so far and on which stream the last one went (what a recorder
 * needs to know which call was the producer). */
int t3d_plan_add_fork_after(t3d_plan* plan, int producer_op, void* from_stream, void* to_stream);
int t3d_launch_count(unsigned long long* count, void** last_stream);
int t3d_plan_add_copy_d2h(t3d_plan* plan, int dst_slot, const void* src, long long bytes, void* stream);
int t3d_plan_add_event_record(t3d_plan* plan, int event_slot, void* stream);
int t3d_plan_end_segment(t3d_plan* plan);
int t3d_plan_num_ops(const t3d_plan* plan, int kind);
int t3d_plan_time_entry(t3d_plan* plan, const char* entry, int on);
int t3d_plan_failed_op(const t3d_plan* plan, int* rc_out);
int t3d_plan_run(t3d_plan* plan, int segment, const unsigned long long* slots, int nslots, void** events, int nevents);

/* The library describes this header (csrc/abi.hip; no reference counterpart: the reference has no FFI to describe).  Both
 * tables are made by the compiler from the declarations above, so a binding that reads them cannot disagree with the code it
 * calls; torchdet3d/_native.py sets every `argtypes` from the first and tests/test_abi.py holds the Python mirrors of the
 * structs to the second.  Pure host functions: no HIP call, no allocation, valid before any device is initialised; the
 * strings are static and live as long as the library.  index runs from 0; T3D_ERR_ARG past the last row (a caller finds the
 * end that way); any output pointer may be NULL.
 * t3d_abi_entry: row `index` of the list of every `int t3d_*(...)` of this header (csrc/abi_entries.h).
 *   name     the entry point;
 *   types    one character per argument, from the declared function type:
 *              i int   l long long   u unsigned long long   f float   d double   p any data pointer
 *            and, for a pointer to one of the structs a caller passes as a struct of its own,
 *              P t3d_prologue*   B t3d_bnbwd*   L t3d_loss_cfg*   S t3d_draw_style*   F t3d_bn_fold*
 *            (an argument of any other type does not compile); the result is always int;
 *   in_step  1 when a recorded step may contain the call (t3d_plan_add_call accepts it), else 0.
 * t3d_abi_struct: row `index` of the list of every `typedef struct {...} t3d_*;` of this header.
 *   name     the typedef;  size = sizeof;
 *   fields   "name:offset:bytes" of every member in declaration order, joined by ',' -- offsetof and sizeof as the compiler
 *            lays the struct out (an array member is one field of its whole extent). */
int t3d_abi_entry(int index, const char** name, const char** types, int* in_step);
int t3d_abi_struct(int index, const char** name, int* size, const char** fields);

#ifdef __cplusplus
}
#endif
#endif /* T3D_H_ */
