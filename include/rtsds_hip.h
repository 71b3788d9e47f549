/*
 * rtsds_hip.h -- C ABI of librtsds_hip.so, the MI355X (gfx950 / CDNA4) kernels behind the
 * RTSDS hot path (BiSeNet / DeepLabV2 forward+backward + adversarial DA discriminator step).
 *
 * The reference (sina-behnam/RTSDS @ 2024-08-07) is pure PyTorch: every kernel on its hot
 * path is an implicit ATen op reached through torch.nn.  Each entry point below names the
 * reference call site(s) whose ATen kernel it replaces.
 *
 * Conventions:
 *  - Activations are NHWC ("channels_last"), dtype RTSDS_F32 or RTSDS_BF16; weights are
 *    [Cout][KH][KW][Cin] in the same dtype; statistics, biases, losses and optimizer state
 *    are fp32.
 *  - Pointers are device pointers owned by the caller (PyTorch caching allocator).  The
 *    library never allocates or frees; scratch comes in as (ws, ws_bytes).
 *  - `stream` is a hipStream_t passed as void*.  Every call is stream-ordered, stateless,
 *    re-entrant and performs no host synchronisation (graph-capture safe).
 *  - Return value: RTSDS_OK or one of the RTSDS_ERR_* codes; the Python layer raises.
 */
#ifndef RTSDS_HIP_H
#define RTSDS_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

enum { RTSDS_F32 = 0, RTSDS_BF16 = 1, RTSDS_F16 = 2 /* the gradient wire only: rtsds_cast, optimizer grad_dtype */ };
enum {
  RTSDS_OK = 0,
  RTSDS_ERR_SHAPE = 1,        /* inconsistent / out-of-range shape */
  RTSDS_ERR_UNSUPPORTED = 2,  /* configuration the kernels do not implement */
  RTSDS_ERR_LAUNCH = 3,       /* HIP launch failure */
  RTSDS_ERR_WORKSPACE = 4     /* ws_bytes smaller than the *_workspace() query */
};
enum { RTSDS_ACT_NONE = 0, RTSDS_ACT_RELU = 1, RTSDS_ACT_LEAKY = 2, RTSDS_ACT_SIGMOID = 3 };
#define RTSDS_ACCUMULATE 0x100 /* conv fwd flag: y += conv(...) (ASPP sum, deeplabv2.py:62-66) */
/* conv fwd (act) / wgrad (accumulate) flag: x is already stored with the padded channel pitch
 * the GEMM gathers (rtsds_conv2d_input_pitch: 19 -> 32 for the discriminator's class-probability
 * input, written by rtsds_upsoftmax_fwd; 3 -> 4 for the image of the stem / spatial-path convs,
 * written by rtsds_nchw_to_nhwc_pad) and zero in channels c..pitch-1: the internal pad pass is
 * skipped.  Rejected (RTSDS_ERR_UNSUPPORTED) where the pitch is c itself.                   */
#define RTSDS_INPUT_PADDED 0x400
/* conv dgrad flag (rtsds_conv2d_dgrad: accumulate; _act / _bnstats: act): w is the packed
 * copy rtsds_conv2d_dgrad_pack_many wrote for this descriptor, not the [Cout][KH][KW][Cin]
 * weight -- the per-call repack is skipped.                                                 */
#define RTSDS_WEIGHT_PACKED 0x800

typedef struct {
  int n, h, w, c;   /* input  [n][h][w][c]                                     */
  int ho, wo, k;    /* output [n][ho][wo][k]                                   */
  int kh, kw;       /* filter size                                             */
  int sh, sw;       /* stride                                                  */
  int ph, pw;       /* zero padding                                            */
  int dh, dw;       /* dilation                                                */
  int dtype;        /* RTSDS_F32 / RTSDS_BF16 for x, w, y                      */
} rtsds_conv_desc;

/* ---------------------------------------------------------------- convolution
 * Replaces nn.Conv2d (ATen convolution fwd / grad_input / grad_weight) at
 * build_bisenet.py:11-12,38,65,67,99-100,109-110,117; torchvision ResNet convs reached via
 * build_contextpath.py:19-24; deeplabv2.py:13,19,24,56,73,99; model.py:54-58,69-70.
 * Implicit GEMM on MFMA (bf16: v_mfma_f32_16x16x32_bf16, f32: v_mfma_f32_16x16x4_f32).  */

/* y = act(conv(x, w) + bias [+ y if act & RTSDS_ACCUMULATE]).  bias may be NULL (fp32 [k]).
 * bn_stats (may be NULL; act must be NONE): receives the following BatchNorm's per-tile
 * partial statistics, fp32 [k][rtsds_conv2d_fwd_stats_tiles(d)][count, mean, M2, 0] (channel-major), consumed
 * by rtsds_bn_fwd(stats_part=...) -- the statistics pass over y is then skipped.
 * ws >= rtsds_conv2d_fwd_workspace(d) (non-zero only when Cin needs channel padding).   */
size_t rtsds_conv2d_fwd_workspace(const rtsds_conv_desc* d);
/* Channel pitch of x that the forward / weight-gradient gathers of d read (0: bad descriptor). */
int rtsds_conv2d_input_pitch(const rtsds_conv_desc* d);
int rtsds_conv2d_fwd_stats_tiles(const rtsds_conv_desc* d);
int rtsds_conv2d_fwd(const rtsds_conv_desc* d, const void* x, const void* w, const float* bias,
                     void* y, int act, float* bn_stats, void* ws, size_t ws_bytes, void* stream);
/* Eval-mode conv + BatchNorm(running stats) (+ residual) (+ act) in one launch (inference
 * path of build_bisenet.py:16-18 ConvBlock, torchvision BasicBlock / Bottleneck,
 * deeplabv2.py:32-47): y = act(conv(x, w) * scale[k] + shift[k] + res), res NHWC like y (may
 * be NULL); scale / shift from rtsds_bn_fold.  Same workspace as rtsds_conv2d_fwd.         */
int rtsds_conv2d_fwd_bn(const rtsds_conv_desc* d, const void* x, const void* w, const float* scale,
                        const float* shift, const void* res, void* y, int act, void* ws, size_t ws_bytes,
                        void* stream);
/* rtsds_conv2d_fwd_bn (no residual) writing y as a channel slice of a wider NHWC tensor: row
 * pitch ldy elements (>= d->k; y 16-B aligned, ldy and d->k multiples of 8 for bf16 / 4 for f32)
 * -- the inference spatial path writes its output straight into the fusion module's
 * concatenated input (build_bisenet.py:153, :72).  RTSDS_ERR_UNSUPPORTED outside the
 * implicit-GEMM route (the caller then writes a plain tensor and copies).                   */
int rtsds_conv2d_fwd_bn_ld(const rtsds_conv_desc* d, const void* x, const void* w, const float* scale,
                           const float* shift, void* y, long ldy, int act, void* ws, size_t ws_bytes, void* stream);
/* Inference stem: eval conv + BatchNorm(running stats) + act + MaxPool2d(3, 2, pool_pad) in one
 * launch (torchvision ResNet conv1 -> bn1 -> relu -> maxpool, deeplabv2.py:106-110): y is the
 * pooled [n][hp][wp][k] NHWC output (hp / wp from the caller: floor or ceil mode); windows
 * skip positions outside the conv output.  Equal to rtsds_conv2d_fwd_bn + rtsds_maxpool_fwd.
 * RTSDS_ERR_UNSUPPORTED outside the 3-channel 7x7 stride-2 image conv with 64 outputs (bf16).
 * Same workspace as rtsds_conv2d_fwd.                                                       */
int rtsds_conv2d_fwd_bn_maxpool(const rtsds_conv_desc* d, const void* x, const void* w, const float* scale,
                                const float* shift, void* y, int act, int hp, int wp, int pool_pad, void* ws,
                                size_t ws_bytes, void* stream);
/* dx (+)= conv_transpose(dy, w) (accumulate != 0: dx += ...).  Needs ws >=
 * rtsds_conv2d_dgrad_workspace(d).  Strides 1 and 2 only.                               */
size_t rtsds_conv2d_dgrad_workspace(const rtsds_conv_desc* d);
/* Pre-packed data-gradient weights: bytes of d's packed copy (0: its route reads w as is --
 * pooled / narrow 1x1 -- and takes no RTSDS_WEIGHT_PACKED); pack_many writes the packed copies
 * wt[i] of count convs (descs[i], weights w[i] in [Cout][KH][KW][Cin]) in one launch per 16
 * segments -- the optimizer's per-step refresh after its update (optim.py).                 */
size_t rtsds_conv2d_dgrad_pack_bytes(const rtsds_conv_desc* d);
int rtsds_conv2d_dgrad_pack_many(int count, const rtsds_conv_desc* descs, const void* const* w, void* const* wt,
                                 void* stream);
int rtsds_conv2d_dgrad(const rtsds_conv_desc* d, const void* dy, const void* w, void* dx,
                       int accumulate, void* ws, size_t ws_bytes, void* stream);
/* dx = conv_transpose(dy, w) * act'(x_act): the data gradient of this conv followed by the
 * backward of the ReLU (act 1) / LeakyReLU(0.2) (act 2) that produced its input x_act (NHWC
 * [n][h][w][c], the activation's output) -- the discriminator's conv -> LeakyReLU -> conv
 * chains (model.py:54-58,69-70), applied in the GEMM epilogue (else as a second pass).
 * Values equal rtsds_conv2d_dgrad followed by rtsds_act_bwd.  Same workspace as dgrad.   */
int rtsds_conv2d_dgrad_act(const rtsds_conv_desc* d, const void* dy, const void* w, void* dx, const void* x_act,
                           int act, void* ws, size_t ws_bytes, void* stream);
/* dx = conv_transpose(dy, w), plus -- from the stored dx values -- the backward statistics of
 * the train-mode BatchNorm (+ ReLU / LeakyReLU, act) whose output is this conv's input
 * (ResNet BasicBlock bn1 -> conv2, Bottleneck bn1 -> conv2, bn2 -> conv3): per M tile t and
 * channel ch, part[(ch * tiles + t) * 2 + {0, 1}] = (sum g, sum g (bn_x - mean)),
 * g = dx * act'(bn_x * gamma * invstd + beta - mean * gamma * invstd) -- what rtsds_bn_bwd's
 * first pass computes, handed to rtsds_bn_bwd_part (the BatchNorm backward then skips it).
 * tiles = rtsds_conv2d_dgrad_bnstats_tiles(d); 0 = route not available (bf16, stride 1 and
 * the plain GEMM route only): call rtsds_conv2d_dgrad instead.                             */
int rtsds_conv2d_dgrad_bnstats_tiles(const rtsds_conv_desc* d);
int rtsds_conv2d_dgrad_bnstats(const rtsds_conv_desc* d, const void* dy, const void* w, void* dx, const void* bn_x,
                               const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                               int act, float* part, void* ws, size_t ws_bytes, void* stream);
/* dw (fp32 [k][kh][kw][c]) = sum_pixels dy (x) patch(x); dbias (fp32 [k], may be NULL) =
 * sum_pixels dy.  accumulate != 0 adds into dw / dbias instead of overwriting (gradients go
 * straight into the optimizer's flat gradient arena, replacing autograd's AccumulateGrad).  */
size_t rtsds_conv2d_wgrad_workspace(const rtsds_conv_desc* d);
int rtsds_conv2d_wgrad(const rtsds_conv_desc* d, const void* x, const void* dy, float* dw,
                       float* dbias, int accumulate, void* ws, size_t ws_bytes, void* stream);
/* Deferred split-K reduction of a weight gradient.  rtsds_conv2d_wgrad_deferred launches every
 * kernel of rtsds_conv2d_wgrad except the final reduction of the fp32 split slabs (which stay in
 * ws) into dw, and describes that reduction in *pending (pending->nv == 0: nothing deferred --
 * the call completed dw itself).  rtsds_split_reduce_many then performs up to n pending
 * reductions in ONE launch (the backward pass's wgrads reduced together instead of one small
 * launch each); descs must target distinct dw, and ws must stay allocated until it has run.  */
typedef struct {
  const float* slab;  /* [splits][k * kh * kw * cp] fp32 partials (in the wgrad's workspace) */
  float* dw;          /* [k][kh][kw][c] fp32                                                   */
  long slab_stride;   /* elements between splits                                              */
  int nv;             /* float4 outputs: k * kh * kw * c / 4                                    */
  int cv, cp;         /* c / 4; the slab's (padded) channel pitch                              */
  int splits, accumulate;
} rtsds_split_reduce_desc;
int rtsds_conv2d_wgrad_deferred(const rtsds_conv_desc* d, const void* x, const void* dy, float* dw,
                                float* dbias, int accumulate, void* ws, size_t ws_bytes,
                                rtsds_split_reduce_desc* pending, void* stream);
int rtsds_split_reduce_many(int n, const rtsds_split_reduce_desc* descs, void* stream);
/* Weight gradient of a 3-channel stride-2 image conv (bf16, c = 3, k = 64, 7x7 or 3x3, even w,
 * odd pw; no bias gradient) whose output feeds a train-mode BatchNorm, with that BatchNorm's
 * backward apply fused in: dx = A*g + B*(bn_x - mean) + C (g = bn_dy masked by the activation,
 * rounded to bf16 exactly as rtsds_bn_bwd stores it) is formed per output tile on the way into
 * the MFMA and never written.  bn_dy: the BatchNorm's incoming gradient, bn_x: its input (this
 * conv's output), both NHWC [n][ho][wo][64]; coef: rtsds_bn_bwd_coef's rows.  x: the image
 * (RTSDS_INPUT_PADDED in accumulate: already the 4-channel padded copy).  One fp32 slab per
 * workgroup in ws, summed in workgroup order by the split reduce (deterministic); the deferred
 * form leaves that reduction to rtsds_split_reduce_many.  workspace == 0 / RTSDS_ERR_UNSUPPORTED:
 * geometry not taken, nothing launched -- use rtsds_bn_bwd + rtsds_conv2d_wgrad.              */
size_t rtsds_imgconv_bn_wgrad_workspace(const rtsds_conv_desc* d);
int rtsds_imgconv_bn_wgrad(const rtsds_conv_desc* d, const void* x, const void* bn_dy, const void* bn_x,
                           const float* coef, int act, float* dw, int accumulate, void* ws, size_t ws_bytes,
                           void* stream);
int rtsds_imgconv_bn_wgrad_deferred(const rtsds_conv_desc* d, const void* x, const void* bn_dy, const void* bn_x,
                                    const float* coef, int act, float* dw, int accumulate, void* ws,
                                    size_t ws_bytes, rtsds_split_reduce_desc* pending, void* stream);

/* ---------------------------------------------------------------- batch norm (train/eval)
 * Replaces nn.BatchNorm2d at build_bisenet.py:13,39; torchvision ResNet bn*; deeplabv2.py:14-27,
 * 75,101 (frozen affine, train-mode batch statistics).  x, y, res, dy, dx: NHWC [rows][c]
 * with rows = n*h*w.
 * Forward (training): mean/invstd of the batch are written to save_mean / save_invstd, the
 * running buffers are updated in place with the unbiased variance, momentum m, and
 * *num_batches_tracked (int64, may be NULL) is incremented on the device (PyTorch
 * semantics).  Forward (eval): running stats are used and copied to save_* when non-NULL.
 * y = act(gamma * (x - mean) * invstd + beta [+ res]).  gamma/beta may be NULL (1 / 0).   */
size_t rtsds_bn_workspace(long rows, int c);
/* stats_part (may be NULL): [c][stats_nrb][count, mean, M2, 0] partials from the producing
 * conv (rtsds_conv2d_fwd bn_stats) -- training mode then skips its own statistics pass.   */
int rtsds_bn_fwd(const void* x, const void* res, void* y, long rows, int c, const float* gamma,
                 const float* beta, float* running_mean, float* running_var,
                 long long* num_batches_tracked, float* save_mean,
                 float* save_invstd, float momentum, float eps, int training, int act,
                 const float* stats_part, int stats_nrb, int dtype, void* ws, size_t ws_bytes,
                 void* stream);
/* rtsds_bn_fwd with y's row pitch ldy >= c (ldy == c: rtsds_bn_fwd): y is a channel slice of a
 * wider NHWC tensor -- the spatial path's output written into the fusion module's concatenated
 * input (build_bisenet.py:153,72).  ldy != c: bf16, c % 8 == 0, ldy % 8 == 0.              */
int rtsds_bn_fwd_ld(const void* x, const void* res, void* y, long ldy, long rows, int c,
                    const float* gamma, const float* beta, float* running_mean, float* running_var,
                    long long* num_batches_tracked, float* save_mean, float* save_invstd,
                    float momentum, float eps, int training, int act, const float* stats_part,
                    int stats_nrb, int dtype, void* ws, size_t ws_bytes, void* stream);
/* Eval-mode fold of BatchNorm2d(running stats) into the preceding conv (+ its bias, may be
 * NULL): scale = gamma / sqrt(running_var + eps), shift = beta + (bias - running_mean) * scale
 * (fp32 [c]; gamma / beta may be NULL = 1 / 0).                                            */
int rtsds_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                  const float* running_var, const float* conv_bias, float eps, int c, float* scale,
                  float* shift, void* stream);
/* Backward of the fused BN(+res)(+act) above.  y (post-activation output) gives the
 * activation mask; it may be NULL without a residual for act NONE/RELU/LEAKY, when the mask
 * is recomputed bit-exactly from x, gamma, beta and save_*.  dx, dres (may be NULL),
 * dgamma/dbeta (fp32, may be NULL; overwritten, or added to when accumulate_params != 0).
 * training=0: eval-mode backward (constant stats).                                        */
int rtsds_bn_bwd(const void* dy, const void* x, const void* y, void* dx, void* dres,
                 float* dgamma, float* dbeta, long rows, int c, const float* gamma,
                 const float* beta, const float* save_mean, const float* save_invstd, int training, int act,
                 int accumulate_params, int dtype, void* ws, size_t ws_bytes, void* stream);
/* rtsds_bn_bwd reading dy with row pitch ldy >= c (a channel slice of the concatenated
 * input's gradient; ldy != c: bf16, c % 8 == 0, ldy % 8 == 0).                              */
int rtsds_bn_bwd_ld(const void* dy, long ldy, const void* x, const void* y, void* dx, void* dres,
                    float* dgamma, float* dbeta, long rows, int c, const float* gamma,
                    const float* beta, const float* save_mean, const float* save_invstd, int training,
                    int act, int accumulate_params, int dtype, void* ws, size_t ws_bytes, void* stream);
/* rtsds_bn_bwd's statistics and finalize passes only (no residual, act NONE/RELU/LEAKY, mask
 * from x): dgamma / dbeta exactly as rtsds_bn_bwd, and the coefficient rows of its apply pass,
 * coef = [A | B | C | mean | scale | shift] x c floats (16-byte aligned, caller-owned), with
 * dx = A*g + B*(x - mean) + C and g = dy * act'(x*scale + shift) -- for a consumer that applies
 * them itself (rtsds_imgconv_bn_wgrad).  Workspace as rtsds_bn_bwd.                        */
int rtsds_bn_bwd_coef(const void* dy, const void* x, float* dgamma, float* dbeta, float* coef, long rows, int c,
                      const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                      int training, int act, int accumulate_params, int dtype, void* ws, size_t ws_bytes,
                      void* stream);
/* rtsds_bn_bwd without its statistics pass: part / nrb = the channel-major (sum g,
 * sum g (x - mean)) partials of rtsds_conv2d_dgrad_bnstats (bf16, c % 8 == 0, no residual).  */
int rtsds_bn_bwd_part(const void* dy, const void* x, void* dx, float* dgamma, float* dbeta, long rows, int c,
                      const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                      int training, int act, int accumulate_params, const float* part, int nrb, int dtype, void* ws,
                      size_t ws_bytes, void* stream);

/* Training-mode residual BatchNorm + ReLU, y = relu(bn(x) + res), that keeps one mask bit per
 * element for its backward instead of y (bf16 / fp32, c % 8 == 0).  bits: one byte per 16-byte
 * channel vector of a row, [rows][c / V] with V = 8 (bf16) or 4 (fp32), rtsds_bn_bits_bytes(rows,
 * c, dtype) bytes (0: unsupported); bit j of a byte = (y[ch0 + j] > 0) of the value as stored.
 * rtsds_bn_fwd_bits: rtsds_bn_fwd(training = 1, act = RELU, res != NULL) plus the bits.
 * rtsds_bn_bwd_bits: rtsds_bn_bwd_ld(training = 1, act = RELU, y) with the mask read from bits;
 * dx and dres both wanted.  Results are bit for bit those of the calls named.             */
size_t rtsds_bn_bits_bytes(long rows, int c, int dtype);
int rtsds_bn_fwd_bits(const void* x, const void* res, void* y, uint8_t* bits, long rows, int c, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                      float* save_mean, float* save_invstd, float momentum, float eps, const float* stats_part,
                      int stats_nrb, int dtype, void* ws, size_t ws_bytes, void* stream);
int rtsds_bn_bwd_bits(const void* dy, long ldy, const void* x, const uint8_t* bits, void* dx, void* dres, float* dgamma,
                      float* dbeta, long rows, int c, const float* gamma, const float* beta, const float* save_mean,
                      const float* save_invstd, int accumulate_params, int dtype, void* ws, size_t ws_bytes,
                      void* stream);
/* The two BatchNorms at the end of a residual block with a downsample branch, on tensors of one
 * [rows][c] shape, in three launches per direction: y = relu(bnA(xa) + round(bnB(xb))), where xa is
 * the raw output of the block's last conv and xb of its downsample conv; the rounded inner value
 * is the skip tensor the separate calls store, which is never written.  Bit for bit
 * rtsds_bn_fwd(xb; act NONE) -> rtsds_bn_fwd(xa, res = skip; RELU) and, backward,
 * rtsds_bn_bwd(A: dx = dxa, dres = g) -> rtsds_bn_bwd(B: dy = g, dx = dxb), both in training mode.
 * One rtsds_bn_params per BatchNorm: the forward reads gamma .. eps (stats_part as rtsds_bn_fwd),
 * the backward gamma, beta, save_*, dgamma, dbeta, accumulate.  bits as rtsds_bn_fwd_bits.
 * Workspace: rtsds_bn_pair_workspace(rows, c).                                             */
typedef struct rtsds_bn_params {
  const float *gamma, *beta;
  float *running_mean, *running_var;
  long long* num_batches_tracked;
  float *save_mean, *save_invstd;
  float momentum, eps;
  const float* stats_part;
  int stats_nrb;
  int accumulate;
  float *dgamma, *dbeta;
} rtsds_bn_params;
size_t rtsds_bn_pair_workspace(long rows, int c);
int rtsds_bn_pair_fwd(const void* xa, const void* xb, void* y, uint8_t* bits, long rows, int c,
                      const rtsds_bn_params* pa, const rtsds_bn_params* pb, int dtype, void* ws, size_t ws_bytes,
                      void* stream);
int rtsds_bn_pair_bwd(const void* dy, long ldy, const void* xa, const void* xb, const uint8_t* bits, void* dxa,
                      void* dxb, long rows, int c, const rtsds_bn_params* pa, const rtsds_bn_params* pb, int dtype,
                      void* ws, size_t ws_bytes, void* stream);

/* BatchNorm2d + ReLU + MaxPool2d(3, 2, p in {0,1}) fused -- the ResNet stem bn1 -> relu ->
 * maxpool (build_contextpath.py:15-18 via torchvision resnet.py; deeplabv2.py:106-110, ceil
 * mode via ho / wo).  bf16, c % 8 == 0.  x: the conv output [n][h][w][c]; y: pooled
 * [n][ho][wo][c]; idx: window argmax 0..8 per output element (first maximum in window order,
 * as ATen).  Statistics, running buffers and workspace as rtsds_bn_fwd (rows = n*h*w).  The
 * backward gathers dy_pool through idx inside the BatchNorm backward passes: dx = d(bn+relu)
 * of the pooled gradient; dgamma / dbeta as rtsds_bn_bwd.                                  */
int rtsds_bn_relu_maxpool_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, int ho, int wo,
                              int p, const float* gamma, const float* beta, float* running_mean,
                              float* running_var, long long* num_batches_tracked, float* save_mean,
                              float* save_invstd, float momentum, float eps, int training,
                              const float* stats_part, int stats_nrb, int dtype, void* ws, size_t ws_bytes,
                              void* stream);
int rtsds_bn_relu_maxpool_bwd(const void* dy_pool, const uint8_t* idx, const void* x, void* dx, float* dgamma,
                              float* dbeta, int n, int h, int w, int c, int ho, int wo, int p,
                              const float* gamma, const float* beta, const float* save_mean,
                              const float* save_invstd, int training, int accumulate_params, int dtype,
                              void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- layout / dtype
 * Input images arrive NCHW fp32 from the reference's loaders (datasets/cityscapes.py:62,
 * main.py:69-72).  cast: weight shadows (fp32 master -> bf16) and dtype round trips.
 * copy_channels: torch.cat along channels and its backward split (build_bisenet.py:72,153);
 * accumulate != 0: dst += src (a split slice whose tensor also has another reader).      */
int rtsds_nchw_to_nhwc(const float* x, void* y, int n, int c, int h, int w, int dtype, void* stream);
/* Same, written with channel pitch `pitch` (channels c..pitch-1 zero; pitch 4): the 3-channel
 * image batch in the layout rtsds_conv2d_input_pitch reports for the stem / spatial-path convs,
 * passed to them with RTSDS_INPUT_PADDED (main.py:46-108 loaders -> model input).           */
int rtsds_nchw_to_nhwc_pad(const float* x, void* y, int n, int c, int h, int w, int pitch, int dtype, void* stream);
int rtsds_cast(const void* src, int src_dtype, void* dst, int dst_dtype, long n, void* stream);
int rtsds_copy_channels(const void* src, int src_ld, int src_off, void* dst, int dst_ld, int dst_off,
                        long rows, int cnt, int accumulate, int dtype, void* stream);

/* ---------------------------------------------------------------- pointwise activations
 * act 1 ReLU (build_bisenet.py:77), 2 LeakyReLU(0.2) (model.py:62,73), 3 sigmoid
 * (build_bisenet.py:49,78).  Backward from the forward output y; act 0 = dx = alpha*dy
 * (GradientReversalFunction, model.py:9-17).                                              */
int rtsds_act_fwd(const void* x, void* y, long n, int act, int dtype, void* stream);
int rtsds_act_bwd(const void* dy, const void* y, void* dx, long n, int act, float alpha, int dtype,
                  void* stream);

/* ---------------------------------------------------------------- pooling
 * MaxPool2d (build_contextpath.py:21 via torchvision; deeplabv2.py:79 ceil_mode -- the
 * caller sizes ho/wo).  idx: uint8 tap index per output, consumed by the backward; NULL for
 * inference (3x3 windows with 16-B channel vectors only, else RTSDS_ERR_UNSUPPORTED).     */
int rtsds_maxpool_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, int ho,
                      int wo, int k, int s, int p, int dtype, void* stream);
int rtsds_maxpool_bwd(const void* dy, const uint8_t* idx, void* dx, int n, int h, int w, int c,
                      int ho, int wo, int k, int s, int p, int dtype, void* stream);
/* Global average pool over H*W (build_bisenet.py:46,75; build_contextpath.py:27-28;
 * model.py:63,82).  y: [n][c].  ws: rtsds_gap_workspace(n, hw, c) bytes (row-slice
 * partials of the two-stage reduction; also used by rtsds_chscale_bwd's da).              */
size_t rtsds_gap_workspace(int n, long hw, int c);
int rtsds_gap_fwd(const void* x, void* y, int n, long hw, int c, int dtype, void* ws, size_t ws_bytes,
                  void* stream);
/* dx (+)= broadcast(dy) / hw; accumulate: add into dx (the gradient another reader of x already
 * wrote there -- functional.GradJoin; same roundings as a separate elementwise add).          */
int rtsds_gap_bwd(const void* dy, void* dx, int n, long hw, int c, int accumulate, int dtype, void* stream);

/* ---------------------------------------------------------------- channel attention
 * mode 0: y = x*a[n][c] (build_bisenet.py:52,149); mode 1: y = x*a + x (build_bisenet.py:79-80).
 * Backward: dx (may be NULL), da[n][c] = sum_hw dy*x (may be NULL; needs
 * ws = rtsds_gap_workspace(n, hw, c) bytes).                                              */
/* Inference tail of FeatureFusionModule + the final 1x1 conv (build_bisenet.py:75-80, 167), two
 * launches: out = conv3(f * a + f) + b3 with a = sigmoid(conv2(relu(conv1(GAP(f)) + b1)) + b2);
 * f / out NHWC [n][hw][c] (c = 19 -- the class maps -- and hw a multiple of the 16-B vector length,
 * else RTSDS_ERR_UNSUPPORTED); w1..w3 [c][c] in the compute dtype, biases fp32 (NULL = 0).  Needs
 * ws >= rtsds_ffm_head_eval_workspace(n, hw, c) bytes (the GAP partials).                     */
size_t rtsds_ffm_head_eval_workspace(int n, long hw, int c);
int rtsds_ffm_head_eval(const void* f, const void* w1, const float* b1, const void* w2, const float* b2,
                        const void* w3, const float* b3, void* out, int n, long hw, int c, int dtype, void* ws,
                        size_t ws_bytes, void* stream);
int rtsds_chscale_fwd(const void* x, const void* a, void* y, int n, long hw, int c, int mode,
                      int dtype, void* stream);
int rtsds_chscale_bwd(const void* dy, const void* x, const void* a, void* dx, void* da, int n,
                      long hw, int c, int mode, int dtype, void* ws, size_t ws_bytes, void* stream);
/* Two mode-0 scales in a row, y = round(round(x * a) * b) with a, b [n][c] (BiSeNet's
 * cx2 = (f4 * att2) * tail, build_bisenet.py:52,149), without the intermediate tensor: the forward
 * is one launch, the backward one pixel pass (dx, both gradients' slice partials) and one final
 * launch for da / db.  Every result equals two rtsds_chscale_fwd / rtsds_chscale_bwd calls' bit
 * for bit.  c a multiple of the 16-B vector length and 16-B aligned tensors only
 * (RTSDS_ERR_UNSUPPORTED otherwise: the caller runs the two calls); dx must not alias dy or x;
 * ws: 2 * rtsds_gap_workspace(n, hw, c) bytes.                                               */
int rtsds_chscale2_fwd(const void* x, const void* a, const void* b, void* y, int n, long hw, int c,
                       int dtype, void* stream);
int rtsds_chscale2_bwd(const void* dy, const void* x, const void* a, const void* b, void* dx, void* da,
                       void* db, int n, long hw, int c, int dtype, void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- bilinear resize
 * F.interpolate(mode='bilinear', align_corners=False) (build_bisenet.py:151-152,158-159,166;
 * deeplabv2.py:126; model.py:23).  scale = in/out (size=) or 1/scale_factor, in fp32 as
 * ATen computes it.  The output (forward) / incoming grad (backward) may be a channel slice
 * of a wider NHWC tensor: pixel pitch *_ld (0 = c), channel offset *_off.               */
int rtsds_bilinear_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo,
                       float scale_h, float scale_w, int y_ld, int y_off, int dtype, void* stream);
/* Inference: rtsds_bilinear_fwd of (x * s1) * s2 (s1 / s2: optional [n][c] channel scales in the
 * activation dtype, each product rounded to it as rtsds_chscale_fwd mode 0 stores it) -- the
 * attention refinement's channel scales (build_bisenet.py:52-53, 157-159) folded into the
 * eval forward's resize.  Upsampling (ho >= hi) with c, y_ld, y_off multiples of a 16-B vector
 * only; RTSDS_ERR_UNSUPPORTED otherwise (the caller scales and resizes separately).      */
int rtsds_bilinear_fwd_scaled(const void* x, const void* s1, const void* s2, void* y, int n, int hi, int wi,
                              int c, int ho, int wo, float scale_h, float scale_w, int y_ld, int y_off,
                              int dtype, void* stream);
/* Backward = separable two-pass gather (W then H) through an fp32 workspace of
 * rtsds_bilinear_bwd_workspace() bytes; deterministic (no atomics).                      */
size_t rtsds_bilinear_bwd_workspace(int n, int hi, int wi, int c, int ho, int wo);
int rtsds_bilinear_bwd(const void* dy, void* dx, int n, int hi, int wi, int c, int ho, int wo,
                       float scale_h, float scale_w, int dy_ld, int dy_off, int dtype, void* ws,
                       size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- adaptive average pool
 * F.adaptive_avg_pool2d(x, (ho, wo)) of adversarial_train_2 (train.py:410,438,445): window
 * rows [floor(o*hi/ho), ceil((o+1)*hi/ho)), same for columns (ATen semantics), NHWC.
 * Backward gathers each input pixel's share of every window containing it (no atomics).   */
int rtsds_adaptive_avgpool_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo,
                               int dtype, void* stream);
int rtsds_adaptive_avgpool_bwd(const void* dy, void* dx, int n, int hi, int wi, int c, int ho, int wo,
                               int dtype, void* stream);

/* ---------------------------------------------------------------- softmax / losses
 * Logits addressed by element strides (sn, sc, shw) per (image, channel, pixel): NHWC and
 * NCHW both work.  Softmax over channels (train.py:225,245,256) writes NHWC with pitch
 * y_ld >= c (extra channels zeroed).                                                      */
int rtsds_softmax_fwd(const void* x, long sn, long sc, long shw, void* y, int y_ld, int n, long hw,
                      int c, int dtype, void* stream);
int rtsds_softmax_bwd(const void* dy, const void* y, int ld, void* dx, long sn, long sc, long shw,
                      int n, long hw, int c, int dtype, void* stream);
/* nn.CrossEntropyLoss(ignore_index) mean over valid pixels (main.py:124-130).  The forward
 * leaves the valid count at ((float*)ws)[2048]; pass that pointer as `count` to the bwd.  */
size_t rtsds_ce_workspace(void);
/* ws + 2048 floats holds (valid count C, loss sum S); rtsds_ce_finish sets loss = S / C after
 * the caller summed C over data-parallel ranks (the backward reads the same C).           */
int rtsds_ce_finish(const void* ws, float* loss, void* stream);
int rtsds_ce_fwd(const void* x, long sn, long sc, long shw, const int64_t* target, float* loss, int n,
                 long hw, int c, int ignore_index, int dtype, void* ws, size_t ws_bytes, void* stream);
int rtsds_ce_bwd(const void* x, long sn, long sc, long shw, const int64_t* target,
                 const float* grad_loss, const float* count, void* dx, int n, long hw, int c,
                 int ignore_index, int dtype, void* stream);
/* nn.CrossEntropyLoss(weight, ignore_index): loss = sum w[t] (lse - x[t]) / sum w[t] over the valid
 * pixels, d loss / dx = w[t] / sum w * (softmax - onehot).  weight: c fp32 values on the device, never
 * read past c.  Same routes, workspace and rtsds_ce_finish as the unweighted pair; the slot at
 * ws + 2048 floats holds the weight sum (summed over data-parallel ranks by the caller like the
 * count).  All-ones weights give the unweighted call's bits.  Before any launch: RTSDS_ERR_SHAPE
 * for a NULL tensor or weight or c outside [1, 32], RTSDS_ERR_WORKSPACE for a NULL or short ws. */
int rtsds_ce_weighted_fwd(const void* x, long sn, long sc, long shw, const int64_t* target,
                          const float* weight, float* loss, int n, long hw, int c, int ignore_index,
                          int dtype, void* ws, size_t ws_bytes, void* stream);
int rtsds_ce_weighted_bwd(const void* x, long sn, long sc, long shw, const int64_t* target,
                          const float* weight, const float* grad_loss, const float* count, void* dx,
                          int n, long hw, int c, int ignore_index, int dtype, void* stream);
/* nn.BCEWithLogitsLoss() mean (main.py:131-132), fp32.                                  */
int rtsds_bce_fwd(const float* x, const float* target, float* loss, int n, void* stream);
int rtsds_bce_bwd(const float* x, const float* target, const float* grad_loss, float* dx, int n,
                  void* stream);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.Adam step (main.py:116-117) over flat fp32 arenas; grad is multiplied by
 * grad_scale first (data-parallel 1/world).  bf16_shadow (may be NULL) receives bf16(param).
 * grad_dtype: RTSDS_F32, or RTSDS_F16 / RTSDS_BF16 for the all-reduced reduced-precision wire
 * copy of the gradients, read directly (no cast back into the fp32 gradient arena).         */
int rtsds_adam_step(float* param, const void* grad, float* exp_avg, float* exp_avg_sq,
                    void* bf16_shadow, long n, float lr, float beta1, float beta2, float eps,
                    float weight_decay, int step, float grad_scale, int grad_dtype, void* stream);

/* The same update with hyper = {lr, 1 - beta1^step, sqrt(1 - beta2^step)} (fp32, device
 * memory) read by the kernel: a captured hipGraph of the training step replays correct
 * updates while the host advances lr and step between replays.                            */
int rtsds_adam_step_dev(float* param, const void* grad, float* exp_avg, float* exp_avg_sq,
                        void* bf16_shadow, long n, const float* hyper, float beta1, float beta2,
                        float eps, float weight_decay, float grad_scale, int grad_dtype, void* stream);

/* rtsds_adam_step_dev over a run [0, n) of the arena, fused with the pending split-K reductions
 * of the weight gradients inside it (rtsds_conv2d_wgrad_deferred): ONE launch.  descs: n_descs
 * pending reductions, ascending in dw, whose ranges [dw, dw + 4 nv) are disjoint, 16-B aligned
 * and inside [grad, grad + n).  For those ranges the slabs are summed exactly as
 * rtsds_split_reduce_many sums them and the update is applied to the sum at once: the gradient
 * is neither written to nor read from the arena.  desc.accumulate here is a set of flags: bit 0
 * -- the arena holds an earlier contribution, read and added first (earlier + sum, as the reduce
 * does); RTSDS_SLAB_KEEP_GRAD -- the gradient is also stored into the arena.  Every other element
 * of the run gets the plain update, gradient from the arena; each element exactly once, no
 * atomics.  Bit for bit rtsds_split_reduce_many followed by rtsds_adam_step_dev (a clean range
 * skips the reduce's 0 + sum, which differs only for sum = -0 and gives the same p, m, v).
 * max_descs: 0, or a lower cap on n_descs (tests).  RTSDS_ERR_UNSUPPORTED, nothing launched:
 * n_descs above the cap (56 -- the tables travel as kernel arguments), grad_dtype other than
 * RTSDS_F32, a base pointer not 16-B aligned (shadow: 8-B), n >= 2^31 - 4096; RTSDS_ERR_SHAPE:
 * a malformed, unsorted, overlapping or out-of-run descriptor.  The caller then reduces with
 * rtsds_split_reduce_many and calls rtsds_adam_step_dev.                                     */
#define RTSDS_SLAB_KEEP_GRAD 2
int rtsds_adam_step_slabs(float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* bf16_shadow,
                          long n, const float* hyper, float beta1, float beta2, float eps,
                          float weight_decay, float grad_scale, int grad_dtype, int n_descs,
                          const rtsds_split_reduce_desc* descs, int max_descs, void* stream);
/* buf[lo[i] .. hi[i]) = 0 for count ranges (host arrays, floats), one launch per 128 ranges:
 * the optimizer's zero_grad over the gradient ranges written since the last one.
 * RTSDS_ERR_SHAPE: a NULL pointer with count > 0, lo < 0, hi < lo or a range of 2^31 floats. */
int rtsds_zero_ranges(float* buf, int count, const long* lo, const long* hi, void* stream);

/* torch.optim.SGD step (main.py:118-120) over a flat fp32 arena: d = grad*grad_scale
 * (+ weight_decay*param); with momentum, buf = d on the first step (first != 0), else
 * buf = momentum*buf + (1-dampening)*d; d = nesterov ? d + momentum*buf : buf;
 * param -= lr*d.  hyper (device fp32 {lr, first}, may be NULL) overrides lr / first for
 * hipGraph replays.  bf16_shadow (may be NULL) receives bf16(param).                       */
int rtsds_sgd_step(float* param, const void* grad, float* momentum_buf, void* bf16_shadow,
                   long n, const float* hyper, float lr, float momentum, float dampening,
                   float weight_decay, int nesterov, int first, float grad_scale, int grad_dtype, void* stream);

/* Mean-teacher (EMA) update over a flat fp32 arena (no counterpart in the reference): per
 * element t = t + w * (s - t) as three separately rounded fp32 operations (subtract, multiply,
 * add; never an FMA), so it can be restated exactly; w = float32(1 - decay) from the host.
 * teacher_bf16_shadow (may be NULL) receives bf16(t), round to nearest even, in the same pass.
 * 16-byte accesses when the three pointers are 16-byte aligned, element by element otherwise.
 * rtsds_ema_many: the same update (no shadow) in one launch over count segments outside an arena
 * (BatchNorm running statistics); teacher / student / numel are DEVICE tables of count entries.
 * Neither synchronises, allocates or touches the host.                                      */
int rtsds_ema_step(float* teacher, const float* student, void* teacher_bf16_shadow, long n, float w,
                   void* stream);
int rtsds_ema_many(int count, float* const* teacher, const float* const* student, const long* numel,
                   float w, void* stream);

/* ---------------------------------------------------------------- metrics
 * argmax over channels, first maximum wins (train.py:102-106,272-275; validation.py:51).
 * out (int64 [n*hw]) may be NULL; if target and correct are given, *correct += #matches.
 * confusion: hist[nc*nc] += bincount(nc*label + pred) for 0 <= label < nc (utils.py:52-58). */
int rtsds_argmax(const void* x, long sn, long sc, long shw, int64_t* out, const int64_t* target,
                 unsigned long long* correct, int n, long hw, int c, int dtype, void* stream);
int rtsds_confusion(const int64_t* label, const int64_t* pred, unsigned long long* hist, long total,
                    int nc, void* stream);

/* ---------------------------------------------------------------- fused upsample + CE
 * Replaces, for nheads (<= 4) low-resolution NHWC logit maps of the same geometry
 * [n][hl][wl][c] (c <= 32), the chain F.interpolate(bilinear, align_corners=False) to
 * [n][c][H][W] -> nn.CrossEntropyLoss(ignore_index) per head -> (head 0) argmax == target
 * pixel count: build_bisenet.py:151-152,158-159,166, deeplabv2.py:126, train.py:86-106.
 * logits / dlogits: host arrays of nheads device pointers.  scale_h/w: ATen source scales
 * (in/out for size=, 1/scale_factor for scale_factor=; upsampling only, <= 1).
 * Forward writes loss[nheads] (mean over non-ignored pixels; may be NULL) and *loss_sum (their
 * sum in head order; may be NULL), adds the head-0 argmax matches to *correct (may be NULL;
 * overwrites it instead when want_grad carries RTSDS_UPCE_SET_CORRECT, so the caller need not
 * zero it) and, when want_grad & 1, keeps unscaled low-res gradient partials in ws.  Backward:
 * dlogits[h] = grad_loss[h * grad_stride] * d loss[h] / d logits[h] from those partials (ws
 * must be the forward's; grad_stride 0 = one upstream gradient for loss_sum).  Full-resolution logits are never materialised.  workspace()
 * returns 0 for geometries the fused path does not cover.                                 */
#define RTSDS_UPCE_SET_CORRECT 2
size_t rtsds_upce_workspace(int nheads, int n, int hl, int wl, int c, int H, int W, float scale_h,
                            float scale_w);
int rtsds_upce_fwd(int nheads, const void* const* logits, const int64_t* target, int n, int hl,
                   int wl, int c, int H, int W, float scale_h, float scale_w, int ignore_index,
                   float* loss, float* loss_sum, unsigned long long* correct, int want_grad,
                   int dtype, void* ws, size_t ws_bytes, void* stream);
/* Data-parallel global mean: ws starts with float stat[1 + nheads] = (valid-pixel count,
 * per-head loss sums).  After the caller sums stat[0] over ranks (a 1-element all-reduce),
 * rtsds_upce_finish recomputes loss / loss_sum = this rank's sums / global count, and
 * rtsds_upce_bwd scales by the global count: the ranks' losses and gradients sum to the
 * single-device mean over the gathered batch exactly.                                     */
int rtsds_upce_finish(int nheads, const void* ws, float* loss, float* loss_sum, void* stream);
/* rtsds_upce_fwd with class weights (nn.CrossEntropyLoss(weight)): weight holds c fp32 values on
 * the device and is never read past c.  Per pixel the loss term, the count term (stat[0] becomes
 * the sum of w[t] over the valid pixels) and the gradient factor are multiplied by w[t]; `correct`
 * stays the unweighted match count.  The plan -- tiles, auxiliary wave, LDS, workspace layout --
 * is that of rtsds_upce_fwd at the same geometry (the weights live in registers), so
 * rtsds_upce_workspace, rtsds_upce_finish and rtsds_upce_bwd serve both, and every geometry the
 * unweighted call covers is covered.  All-ones weights give the unweighted bits.  Before any
 * launch: RTSDS_ERR_SHAPE for a NULL logits / target / weight pointer or c outside [1, 32];
 * otherwise the codes of rtsds_upce_fwd.                                                    */
int rtsds_upce_weighted_fwd(int nheads, const void* const* logits, const int64_t* target,
                            const float* weight, int n, int hl, int wl, int c, int H, int W,
                            float scale_h, float scale_w, int ignore_index, float* loss,
                            float* loss_sum, unsigned long long* correct, int want_grad, int dtype,
                            void* ws, size_t ws_bytes, void* stream);
int rtsds_upce_bwd(int nheads, const float* grad_loss, int grad_stride, void* const* dlogits,
                   int n, int hl, int wl, int c, int H, int W, float scale_h, float scale_w,
                   int dtype, const void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- discriminator input
 * softmax(interpolate_bilinear(x)) over classes (train.py:225,245,256) in one pass: x NHWC
 * [n][hi][wi][c], y NHWC [n][ho][wo][y_ld] with channels c..y_ld-1 zero (the padded input of
 * the discriminator's first conv, RTSDS_INPUT_PADDED).  Bit-identical to rtsds_bilinear_fwd
 * followed by the channel softmax.  rtsds_upsoftmax_bwd: dx = resize_adjoint(softmax_bwd(dy,
 * y)) (dy with row pitch dy_ld), bit-identical to the unfused backward chain.  c <= 32.      */
int rtsds_upsoftmax_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo,
                        float scale_h, float scale_w, int y_ld, int dtype, void* stream);
size_t rtsds_upsoftmax_bwd_workspace(int n, int hi, int wi, int c, int ho, int wo);
int rtsds_upsoftmax_bwd(const void* dy, int dy_ld, const void* y, int y_ld, void* dx, int n, int hi,
                        int wi, int c, int ho, int wo, float scale_h, float scale_w, int dtype,
                        void* ws, size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- discriminator input, AdvEnt form
 * The weighted self-information maps of ADVENT (Vu et al., CVPR 2019: prob_2_entropy,
 * -p log2(p + 1e-30) / log2(c), here without the epsilon) of the resized head, in
 * rtsds_upsoftmax_fwd's layout: x NHWC [n][hi][wi][c], y NHWC [n][ho][wo][y_ld], c <= y_ld <= 32,
 * channels c..y_ld-1 exact zeros.  Per output pixel, z = the bilinear resize (align_corners =
 * False) rounded to the activation dtype T exactly as rtsds_bilinear_fwd stores it (the logits
 * rtsds_upsoftmax_fwd starts from, bit for bit), then in fp32
 *   d_k = z_k - max z    e_k = expf(d_k)    S = sum_k e_k (class order)    p_k = e_k * (1 / S)
 *   L_k = logf(S) - d_k                     (= -ln p_k >= 0: one logf per pixel, none per class)
 *   I_k = p_k * L_k * fp32(1 / ln c)        and I_k = 0 where e_k == 0 (a class at -inf: 0, not NaN)
 * and y_k = I_k rounded to T; 0 <= I_k <= 1 / (e ln c).
 * rtsds_upselfinfo_bwd, given dy (c channels, row pitch dy_ld) and the same x:
 *   a_k = (L_k - 1) * fp32(1 / ln c)        (= dI_k / dp_k; 0 where e_k == 0)
 *   u_k = dy_k * a_k
 *   dz_j = p_j * (u_j - sum_k p_k u_k)      (sum in class order)
 *   dx   = resize adjoint of dz             (width adjoint, then the vertical pass of
 *                                            rtsds_bilinear_bwd)
 * p and L are formed again from x by the forward's own code (I does not determine p: -p ln p is
 * not monotone), so nothing of the forward's output is read; dz stays fp32 until the adjoint has
 * summed it and only dx is rounded to T.  Fixed summation order, no atomics, no memset, no host
 * synchronisation: two runs give equal bits and both entries capture into a graph.
 * RTSDS_ERR_SHAPE: c outside [2, 32], y_ld outside [c, 32], dy_ld < c, an empty tensor;
 * RTSDS_ERR_WORKSPACE: ws_bytes below the query; RTSDS_ERR_UNSUPPORTED: another dtype, more
 * than INT_MAX tiles, or (backward) an upsampling so steep that the tile of a single input
 * column exceeds the kernel's LDS (some 370 output columns per input column at 32 classes). */
int rtsds_upselfinfo_fwd(const void* x, void* y, int n, int hi, int wi, int c, int ho, int wo,
                         float scale_h, float scale_w, int y_ld, int dtype, void* stream);
size_t rtsds_upselfinfo_bwd_workspace(int n, int hi, int wi, int c, int ho, int wo);
int rtsds_upselfinfo_bwd(const void* dy, int dy_ld, const void* x, void* dx, int n, int hi, int wi,
                         int c, int ho, int wo, float scale_h, float scale_w, int dtype, void* ws,
                         size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- multi-scale / flip evaluation
 * One pass of the summed-probability evaluation protocol: p = softmax(interpolate_bilinear(x))
 * exactly as rtsds_upsoftmax_fwd forms it (same geometries, c <= 32), kept in fp32 (fp32 mode:
 * bit-identical to rtsds_upsoftmax_fwd's output; bf16 mode: its value before the bf16 rounding),
 * stored into (accumulate == 0) or added onto (accumulate != 0: one fp32 add of the rounded
 * product, never an FMA) acc, fp32 NHWC [n][ho][wo][c] with dense pitch c.  flip != 0 stores
 * the pixel computed at output column ow at column wo - 1 - ow (un-mirrors the prediction of a
 * mirrored image).  pred (int64 [n][ho][wo], may be NULL) receives the argmax over classes of
 * the updated acc row, first maximum wins, at the same column.  One owner per output pixel:
 * no atomics, no host synchronisation (graph-capture safe).                                 */
int rtsds_upsoftmax_acc(const void* x, float* acc, int64_t* pred, int n, int hi, int wi, int c,
                        int ho, int wo, float scale_h, float scale_w, int flip, int accumulate,
                        int dtype, void* stream);

/* ---------------------------------------------------------------- pseudo-labels (self-training)
 * No counterpart in the reference (it never trains on target pixels).  Class-balanced
 * self-training keeps, per class, the most confident share of the pixels predicted as that
 * class; the two entries below turn the fp32 probability sum rtsds_upsoftmax_acc leaves into
 * such labels without a host round trip per pixel.
 * rtsds_conf_hist: acc = total pixels x c contiguous fp32.  Per pixel k = argmax over classes
 *   (first maximum wins, NaN handled as rtsds_argmax does), conf = acc[k] * inv (one fp32
 *   multiply; inv = 1 / number of summed passes), b = floor(conf * bins) clamped to
 *   [0, bins - 1] (a conf that is not > 0: bin 0).  hist[k * bins + b] += 1 -- hist (uint64
 *   [c][bins]) is ADDED to, never cleared, so it accumulates over batches; pred[p] = k (uint8)
 *   and cbin[p] = b (uint16), each may be NULL.  2 <= c <= 32; bins a power of two in
 *   [16, 1024] (conf * bins is then exact: the bin is reproducible on the host bit for bit) with
 *   c * (bins + 512) * 4 <= 160 KiB (the workgroup-private histogram plus a 512-pixel tile in
 *   LDS; RTSDS_ERR_UNSUPPORTED otherwise, e.g. c = 32 with bins = 1024).  Integer atomics only:
 *   deterministic.
 * rtsds_pseudo_select: out[p] (int64) = pred[p] if cbin[p] >= tbin[pred[p]] else ignore_index;
 *   tbin = c device ints (a value >= bins keeps nothing of that class).
 * Neither synchronises, allocates or touches the host (graph-capture safe).               */
int rtsds_conf_hist(const float* acc, unsigned long long* hist, uint8_t* pred, uint16_t* cbin,
                    long total, int c, int bins, float inv, void* stream);
int rtsds_pseudo_select(const uint8_t* pred, const uint16_t* cbin, const int* tbin, int64_t* out,
                        long total, int c, int ignore_index, void* stream);

/* rtsds_upsample_pseudo: the three entries rtsds_upsoftmax_acc (accumulate = 0, flip = 0) ->
 *   rtsds_conf_hist (inv = 1, no histogram) -> rtsds_pseudo_select in one pass over the
 *   low-resolution head x (NHWC [n][hi][wi][c], geometry as rtsds_upsoftmax_acc): per output
 *   pixel the probabilities stay in registers, pred[p] = k (uint8) and cbin[p] = b (uint16) by
 *   rtsds_conf_hist's rule, labels[p] (int64) = b >= tbin[k] ? k : ignore_index.  Each output
 *   may be NULL, not all three; labels needs tbin (c device ints).  2 <= c <= 32, bins a power
 *   of two in [16, 1024].  Equal to the chain bit for bit; the fp32 probability tensor is never
 *   written.  For the online (mean-teacher) labels of selftrain.TeacherLoader.               */
int rtsds_upsample_pseudo(const void* x, uint8_t* pred, uint16_t* cbin, const int* tbin, int64_t* labels,
                          int n, int hi, int wi, int c, int ho, int wo, float scale_h, float scale_w,
                          int bins, int ignore_index, int dtype, void* stream);

/* ---------------------------------------------------------------- prediction (painted frames)
 * No counterpart in the reference (it never writes a prediction out).
 * rtsds_upsample_paint: the low-resolution head x (NHWC [n][hi][wi][c], fp32 or bf16, geometry as
 *   rtsds_upsoftmax_acc) -> a class map and a coloured frame at the output size in one pass.  Per
 *   output pixel p the resized logits are formed as rtsds_bilinear_fwd stores them (the blend of
 *   the four taps rounded to the storage type) and k = their argmax over classes, first maximum
 *   wins, NaN handled as rtsds_argmax does; no softmax (it does not move the argmax).  k equals
 *   the chain rtsds_bilinear_fwd -> rtsds_argmax bit for bit; the resized logits are never written.
 *   ids[p] (uint8 [n][ho][wo], may be NULL) = lut ? lut[k] : k, lut = c device bytes (train id ->
 *   label id).  rgb[p][j] (uint8 HWC [n][ho][wo][3], may be NULL, not both) = palette[k][j] when
 *   alpha_q8 == 256, else (alpha_q8 * palette[k][j] + (256 - alpha_q8) * frame[p][j] + 128) >> 8 in
 *   integers (reproducible on the host bit for bit; alpha_q8 = 0 returns the frame); palette =
 *   device uint8 [c][3], frame = uint8 HWC [n][ho][wo][3] (may be NULL when alpha_q8 == 256 or
 *   rgb is NULL).  No alignment is asked of any byte buffer.  2 <= c <= 32, 0 <= alpha_q8 <= 256.
 *   No synchronisation, allocation or host access (graph-capture safe).                       */
int rtsds_upsample_paint(const void* x, const uint8_t* frame, const uint8_t* palette, const uint8_t* lut,
                         uint8_t* ids, uint8_t* rgb, int n, int hi, int wi, int c, int ho, int wo,
                         float scale_h, float scale_w, int alpha_q8, int dtype, void* stream);

/* rtsds_slide_paint: sliding-window ("tiled") inference at native resolution.  The model ran on
 *   nwin overlapping hw x ww crops of an H x W canvas, for nf frames; x holds their NHWC heads
 *   [nwin * nf][hi][wi][c] (fp32 or bf16), window-major: the head of window k of frame f at index
 *   k * nf + f, so a chunk of windows is a contiguous slice.  Geometry (hi, wi) -> (hw, ww) with
 *   scale_h / scale_w as rtsds_upsoftmax_acc takes them (any geometry that entry accepts).
 *   win = HOST array of nwin triples {y0, x0, flip}, 1 <= nwin <= 64, copied into the kernel's
 *   arguments by the launcher (no device table, nothing to clamp, graph-capture safe); every
 *   window must lie inside the canvas, 0 <= y0 <= H - hw and 0 <= x0 <= W - ww.
 *   Window k's probabilities at its own pixel (oy, ow): p = z[k] * iz exactly as
 *   rtsds_upsoftmax_acc forms them (bf16 mode: the value before any bf16 rounding); with
 *   flip != 0 the pixel computed at window column ow belongs to window column ww - 1 - ow.
 *   Sum at canvas pixel (f, Y, X): the windows covering it in ascending k; s starts as
 *   acc[f][Y][X][:] when accumulate != 0, else as the first covering window's p; every further
 *   window is one fp32 add of the rounded product, never an FMA.  A pixel no window covers has
 *   s = acc (accumulate) or all zeros.  Equal, bit for bit, to rtsds_upsoftmax_acc per window
 *   followed by an fp32 add of each window's tensor onto its slice of the canvas.
 *   acc (fp32 [nf][H][W][c], dense pitch c; may be NULL when accumulate == 0) receives s.
 *   k* = argmax s by rtsds_upsoftmax_acc's pred rule (strictly greater wins, first maximum kept,
 *   no NaN clause).  ids[p] (uint8 [nf][H][W]) = lut ? lut[k*] : k*, rgb[p] (uint8 [nf][H][W][3])
 *   the palette blend over frame -- rtsds_upsample_paint's outputs bit for bit (integer blend,
 *   0 <= alpha_q8 <= 256, frame needed only when blending, no alignment asked of byte buffers).
 *   acc, ids and rgb may each be NULL, not all three; with acc NULL no fp32 canvas is touched.
 *   RTSDS_ERR_SHAPE: nf, a size or nwin < 1, hw > H, ww > W, a window outside the canvas, c
 *   outside [2, 32], alpha_q8 outside [0, 256].  RTSDS_ERR_UNSUPPORTED: nwin > 64 (the caller
 *   chunks: accumulate), a bad dtype, a missing pointer the asked outputs need.  Every check is
 *   made on the host before any HIP call.  One owner per canvas pixel: no atomics; never
 *   synchronises, allocates or touches host memory other than win.                            */
int rtsds_slide_paint(const void* x, const int* win, int nwin, const uint8_t* frame,
                      const uint8_t* palette, const uint8_t* lut, float* acc, uint8_t* ids,
                      uint8_t* rgb, int nf, int hi, int wi, int c, int hw, int ww, int H, int W,
                      float scale_h, float scale_w, int accumulate, int alpha_q8, int dtype,
                      void* stream);

/* ---------------------------------------------------------------- ClassMix (self-training)
 * No counterpart in the reference.  ClassMix (DACS, DAFormer) pastes the pixels of half of the
 * classes of a labelled source image, image and label, onto a target image; here the rest of
 * the label map is the thresholded pseudo-label of rtsds_pseudo_select, formed on the fly.
 * Geometry: n samples; source maps [n][hs][ws]; the window (= target) size h x w, hs >= h and
 * ws >= w; per sample a window origin (y0, x0) = origins[i * origin_pitch + {0, 1}] (device
 * int32, origin_pitch >= 2 ints per row) with 0 <= y0 <= hs - h, 0 <= x0 <= ws - w (a value
 * outside that range is clamped into it: the origins are device data, no access may leave the
 * buffers).  2 <= c <= 32 classes; a label s is a class iff 0 <= s < c.
 * rtsds_class_presence: present[i] (uint32) = OR of 1u << s over the classes s in the window
 *   slab[i][y0 : y0 + h][x0 : x0 + w] (int64).  present need not be cleared by the caller (an
 *   asynchronous memset on the stream precedes the kernel).  Only the window is read.
 * rtsds_classmix: with P = the classes of present[i] (bits >= c dropped), quota =
 *   (|P| + 1) >> 1 and key row perm[i * perm_pitch + k] (device int32, perm_pitch >= c), class
 *   k in P is chosen iff #{j in P : perm[j] < perm[k] or (perm[j] == perm[k] and j < k)} <
 *   quota; chosen[i] (uint32, may be NULL) receives the mask of the chosen classes (P empty: 0).
 *   Per window pixel with s = slab[i][y0 + y][x0 + x] and M = (s is a class and chosen):
 *     out_img[i][y][x] = M ? src[i][y0 + y][x0 + x] : tgt[i][y][x]   (the whole record of
 *                        pix_bytes bytes, bit for bit, pad lane included)
 *     out_lab[i][y][x] = M ? s : (k = pred[i][y][x]) < c and cbin[i][y][x] >= tbin[k] ? k
 *                        : ignore_index                    (int64; rtsds_pseudo_select's rule)
 *     mask[i][y][x]    = M ? 1 : 0                          (uint8, may be NULL)
 *   Images are opaque pixel records, pix_bytes in {6, 8, 12, 16} (bf16 / fp32 with a pixel
 *   pitch of 3 or 4 elements), src [n][hs][ws], tgt and out_img [n][h][w], one form for all
 *   three.  Rows whose target start is a multiple of 8 pixels move in 16-byte vectors when all
 *   bases are 16-byte aligned (pred / mask 8) and the source row start is a multiple of 8 / 2 /
 *   4 / 2 pixels for pix_bytes 6 / 8 / 12 / 16 (8 and 16: any start, with 8-byte source loads);
 *   every other row takes a per-pixel path with the same results.
 * RTSDS_ERR_SHAPE: n, h or w < 1, n > 65535, h > hs or w > ws, c outside [2, 32], a pitch too
 * small.  RTSDS_ERR_UNSUPPORTED: another pix_bytes, a NULL or misaligned pointer.  Neither
 * entry synchronises, allocates or touches the host (graph-capture safe).                    */
int rtsds_class_presence(const int64_t* slab, const int* origins, int origin_pitch, unsigned int* present,
                         int n, int hs, int ws, int h, int w, int c, void* stream);
int rtsds_classmix(const void* src, const int64_t* slab, const void* tgt, const uint8_t* pred,
                   const uint16_t* cbin, const int* tbin, const unsigned int* present, const int* perm,
                   int perm_pitch, const int* origins, int origin_pitch, void* out_img, int64_t* out_lab,
                   uint8_t* mask, unsigned int* chosen, int n, int hs, int ws, int h, int w, int c,
                   int pix_bytes, int ignore_index, void* stream);

/* ---------------------------------------------------------------- input pipeline
 * The reference's per-sample torchvision transforms (main.py:60-108; datasets/cityscapes.py:
 * 56-68, datasets/gta5.py:69-118) on a decoded HWC image in device memory.
 * rtsds_resize_aa: Resize((ho, wo), antialias=True) == F.interpolate(bilinear,
 *   align_corners=False, antialias=True) of the float image, optionally of its horizontal
 *   mirror (flip != 0: RandomHorizontalFlip applied before the resize), with the epilogue of
 *   kind 0: f32 HWC, 1: bf16 HWC (both (v - mean[c]) / std[c] when mean/std are given:
 *   Normalize on the 0-255 scale), 2: int64 label (round half-to-even, clamp to
 *   [clamp_lo, clamp_hi] when clamp_lo <= clamp_hi: IntRangeTransformer).  src_u8 selects a
 *   uint8 (else fp32) source.  dst is the image's slot in an NHWC batch.
 * rtsds_crop_resize_aa: rtsds_resize_aa of the window src[y0 : y0 + hc, x0 : x0 + wc, :] of the
 *   [h][w][c] image, read in place (RandomResizedCrop ahead of the Resize; flip mirrors inside
 *   the window).  Bit-identical to rtsds_resize_aa on a contiguous copy of the window; the
 *   workspace is rtsds_resize_aa_workspace(c, hc, wc, ho, wo).
 * rtsds_crop_resize_nearest: the same window of a [h][w] label (uint8, or int64 when src_i64)
 *   resampled to int64 [ho][wo] with F.interpolate(mode="nearest")'s index rule
 *   (min((int)floorf(o * ((float)in / (float)out)), in - 1)); flip != 0 writes the horizontal
 *   mirror of that result (interpolate, then flip); clamped to [clamp_lo, clamp_hi] when
 *   clamp_lo <= clamp_hi.
 *   Both: RTSDS_ERR_SHAPE for a NULL pointer, a non-positive size, a window not inside
 *   [0, h) x [0, w) or mean / std given singly; RTSDS_ERR_UNSUPPORTED / RTSDS_ERR_WORKSPACE as
 *   rtsds_resize_aa on the window; all before any launch.
 * rtsds_gaussian_blur: GaussianBlur((kx, ky), sigma) of a HWC image (uint8 or fp32 source),
 *   fp32 HWC out, reflect padding.
 * rtsds_gta5_decode: RGB label (HWC uint8) -> train id 0..18 (unmatched colours -> 0).
 * rtsds_color_jitter: torchvision ColorJitter of a HWC RGB image (c == 3, else
 *   RTSDS_ERR_UNSUPPORTED; uint8 or fp32 source with values in [0, bound]), fp32 HWC out; dst may
 *   be src for an fp32 source.  Op ids 0 brightness, 1 contrast, 2 saturation, 3 hue are applied in
 *   `order` (four host ints, a permutation of 0..3); bit k of `mask` switches id k on; fb / fc / fs
 *   >= 0 and fh in [-0.5, 0.5] are the factors torchvision's get_params draws.  Every op clamps
 *   to [0, bound]; hue works on p / bound (bound = 1 is torchvision's float image, 255 the
 *   reference's 0-255 scale).  With contrast on, a first launch reduces the grey mean of the image
 *   as it stands when contrast is applied into the workspace (rtsds_color_jitter_workspace bytes;
 *   not read otherwise, ws may be NULL); the result is bitwise reproducible.  Arguments are
 *   validated before any HIP call.                                                              */
size_t rtsds_resize_aa_workspace(int c, int h, int w, int ho, int wo);
int rtsds_resize_aa(const void* src, int src_u8, int c, int h, int w, void* dst, int kind, int ho, int wo,
                    int flip, const float* mean, const float* std, int clamp_lo, int clamp_hi, void* ws,
                    size_t ws_bytes, void* stream);
int rtsds_crop_resize_aa(const void* src, int src_u8, int c, int h, int w, int y0, int x0, int hc, int wc,
                         void* dst, int kind, int ho, int wo, int flip, const float* mean, const float* std,
                         int clamp_lo, int clamp_hi, void* ws, size_t ws_bytes, void* stream);
int rtsds_crop_resize_nearest(const void* src, int src_i64, int h, int w, int y0, int x0, int hc, int wc,
                              int64_t* dst, int ho, int wo, int flip, int clamp_lo, int clamp_hi, void* stream);
int rtsds_gaussian_blur(const void* src, int src_u8, float* dst, int c, int h, int w, int kx, int ky,
                        float sigma_x, float sigma_y, void* stream);
int rtsds_gta5_decode(const uint8_t* rgb, int64_t* out, int h, int w, void* stream);
size_t rtsds_color_jitter_workspace(int h, int w);
int rtsds_color_jitter(const void* src, int src_u8, float* dst, int c, int h, int w, const int* order,
                       int mask, float fb, float fc, float fs, float fh, float bound, void* ws,
                       size_t ws_bytes, void* stream);

/* ---------------------------------------------------------------- histogram matching
 * Per-channel histogram matching of a decoded HWC RGB uint8 image to a reference image's
 * statistics (Abramov et al. 2020; no reference counterpart), integers only.  For one channel
 * with source counts hs, reference counts hr, inclusive prefix sums Cs, Cr and totals Ns, Nr:
 *   m[v]   = min { t in 0..255 : Cr[t] * Ns >= Cs[v] * Nr }   (64-bit products; v when Ns or Nr is 0)
 *   lut[v] = (v * (256 - A) + m[v] * A + 128) >> 8            A = strength_q8: 0 identity, 256 full
 *   out    = lut[channel][in]
 * rtsds_hist_u8: hist[ch][v] (uint32 [3][256]) = the number of pixels of img ([h][w][3]) whose
 *   channel ch equals v.  hist is zeroed on the stream first (a memset node under capture), then
 *   one launch adds into it with integer atomics: the result does not depend on arrival order.
 * rtsds_hist_match: dst = the matched src in one launch, from the histogram of src and that of
 *   the reference image (which may have another size); every block rebuilds the 768-byte LUT in
 *   LDS, nothing is synchronised with the host.  dst may be src.  lut_out ([3][256] bytes, or
 *   NULL) receives the LUT.  The totals of both histograms must be pixel counts (<= 2^32 - 1).
 * Both: RTSDS_ERR_SHAPE for a NULL pointer (lut_out aside), a non-positive size, h * w above
 *   2^32 - 1 or strength_q8 outside [0, 256]; RTSDS_ERR_UNSUPPORTED for c != 3 or a histogram
 *   pointer that is not 4-B aligned; all before any HIP call.  A 16-B aligned image base takes
 *   the vector path, any other the byte path.                                                   */
int rtsds_hist_u8(const uint8_t* img, int c, int h, int w, unsigned int* hist, void* stream);
int rtsds_hist_match(const uint8_t* src, uint8_t* dst, int c, int h, int w, const unsigned int* hist_src,
                     const unsigned int* hist_ref, int strength_q8, uint8_t* lut_out, void* stream);

/* ---------------------------------------------------------------- Fourier domain adaptation
 * FDA (Yang & Soatto, CVPR 2020; no reference counterpart) of a decoded HWC RGB uint8 image: the
 * amplitude of the (2b+1) x (2b+1) lowest frequencies of the source's 2-D spectrum is replaced by a
 * target image's, the phase is kept.  Only the band changes, so with F the source's DFT
 *   out(y,x) = src(y,x) + 1/(hw) * sum_{|u|,|v| <= b} D(u,v) e^{2 pi i (uy/h + vx/w)}
 *   D = strength * (A_t - A_s) * F / A_s      A_s = |F|, A_t = amp_ref_norm * (hw);
 *                                             D = strength * A_t (zero phase) where A_s == 0
 * and no full-frame transform is made.  Band layout, everywhere: fp32 spec[ch][iu][v][2] (re, im),
 * iu = u + b for u = -b..b, v = 0..b; the other half follows from F(-u,-v) = conj F(u,v).  The
 * amplitude arrays have the same layout without the last axis.
 * rtsds_fda_spectrum: spec (or NULL) = F(u,v) = sum_y sum_x img[y][x][ch] e^{-2 pi i (uy/h + vx/w)}
 *   over the band, amp_norm (or NULL, not both) = |F| / (hw), the size-independent form a bank of
 *   target images stores.  Two launches: every row reduced over x for v = 0..b into the workspace
 *   (rtsds_fda_workspace bytes), those reduced over y for u = -b..b.  No floating-point atomics,
 *   every sum has a fixed order: two runs give the same bits.
 * rtsds_fda_apply: dst = the adapted src in one launch from the source's band spec_src and the
 *   target's normalised amplitudes amp_ref_norm (the target image may have another size).  Per
 *   pixel and channel out = src + (G(y,0).re + 2 sum_{v=1..b} Re(G(y,v) e^{2 pi i vx/w})) / (hw) with
 *   G(y,v) = sum_u D(u,v) e^{2 pi i uy/h}; every block forms the D and G of its rows in its prologue.
 *   dst_u8 == 0: fp32 HWC, clamped to [0, 255]; else uint8 (rintf, then the clamp), and dst may be src.
 * Every twiddle's phase is reduced in integers (u y mod h, v x mod w) before cos / sin are formed.
 * All: c == 3 (else RTSDS_ERR_UNSUPPORTED, as for an fp32 pointer that is not 4-B aligned);
 *   RTSDS_ERR_SHAPE for a NULL image or spectrum pointer, a non-positive size, b outside [1, 64],
 *   2b + 1 > min(h, w), h * w > 2^24, strength outside [0, 1] or NaN; RTSDS_ERR_WORKSPACE for a
 *   NULL or short workspace (rtsds_fda_workspace returns 0 for a shape it refuses); all before any
 *   HIP call.  A 16-B aligned image base with w % 4 == 0 takes the dword path (12 bytes per lane),
 *   anything else the byte path, with the same bits.                                              */
size_t rtsds_fda_workspace(int h, int w, int b);
int rtsds_fda_spectrum(const uint8_t* img, int c, int h, int w, int b, float* spec, float* amp_norm, void* ws,
                       size_t ws_bytes, void* stream);
int rtsds_fda_apply(const uint8_t* src, void* dst, int dst_u8, int c, int h, int w, int b, const float* spec_src,
                    const float* amp_ref_norm, float strength, void* stream);

/* ---------------------------------------------------------------- knowledge distillation
 * Soft-target loss between two low-resolution class maps (Hinton et al., 2015; no reference
 * counterpart): student s [n][hs][ws][c] and teacher t [n][ht][wt][c], NHWC, each fp32 or bf16 by
 * its own dtype code, 2 <= c <= 32.  The teacher is resampled onto the student's grid inside the
 * kernel: bilinear, align_corners = False, not antialiased, any ratio up or down; scale_h / scale_w
 * are ATen's source scales ht / hs and wt / ws in fp32, the four taps are blended in fp32 and the
 * blend is not rounded to a storage type; a tap of weight zero is left out, so equal sizes give the
 * identity, also for a teacher logit of -inf (a masked class).  Per student
 * pixel, with a = s * inv_temp, b = u * inv_temp (u the resampled teacher row, inv_temp = fp32(1/T)),
 * q = softmax(a), p = softmax(b):
 *   KL = sum_k p_k (log p_k - log q_k)      a term with p_k == 0 contributes 0
 * Both softmaxes are one expression, so t == s gives exactly 0.  Neither u nor p, q reach memory.
 * rtsds_distill_fwd: one launch; workgroup i leaves the KL sum of its tile in the workspace, and,
 *   when want_grad, the residual q - p as fp32 [n][hs][ws][c] behind the partials.  agree (or NULL):
 *   a device counter that receives += the number of pixels whose first maximum (torch.argmax's rule)
 *   of s equals that of u; integer atomics only.
 * rtsds_distill_finish: loss = coef * (sum of the partials), summed in a fixed order in fp64: the
 *   same bits on every run.  The caller passes coef = T^2 / (n hs ws world).
 * rtsds_distill_bwd: dx [n][hs][ws][c] (dtype) = cast(fp32(*grad_loss * coef_g) * (q - p)) from the
 *   residual of a want_grad forward on the same workspace; coef_g = T / (n hs ws world).
 * None synchronises, allocates or touches the host.  Before any HIP call: RTSDS_ERR_SHAPE for a NULL
 * tensor, a size < 1, c outside [2, 32], a tensor of 2^31 elements or more, a scale, inv_temp or
 * coefficient that is not positive and finite; RTSDS_ERR_UNSUPPORTED for another dtype code, a
 * tensor not aligned to its element, a workspace not 16-B aligned; RTSDS_ERR_WORKSPACE for a NULL or
 * short workspace (rtsds_distill_workspace bytes; 0 for a shape it refuses).                       */
size_t rtsds_distill_workspace(int n, int hs, int ws, int c, int ht, int wt);
int rtsds_distill_fwd(const void* s, int s_dtype, const void* t, int t_dtype, int n, int hs, int ws, int c, int ht, int wt,
                      float scale_h, float scale_w, float inv_temp, int want_grad, unsigned long long* agree, void* wsp,
                      size_t ws_bytes, void* stream);
int rtsds_distill_finish(const void* wsp, size_t ws_bytes, int n, int hs, int ws, double coef, float* loss, void* stream);
int rtsds_distill_bwd(const void* wsp, size_t ws_bytes, const float* grad_loss, double coef_g, void* dx, int dtype, int n, int hs,
                      int ws, int c, void* stream);

/* ---------------------------------------------------------------- target entropy minimisation
 * An unsupervised penalty on a low-resolution class map (no reference counterpart): x [n][h][w][c]
 * dense NHWC, fp32 or bf16, aligned to its element only, 2 <= c <= 32.  Per pixel, with logits z:
 *   d = z - max z, e = exp d, Z = sum e, p = e / Z, log p = d - log Z
 *   H = -sum_k p_k log p_k      a term with p_k == 0 counts 0, so a class at -inf gives 0, not NaN
 *   h = min(H * fp32(1 / ln c), 1)     the normalised entropy, in [0, 1]
 *   S = sum_k p_k^2
 *   RTSDS_ENTROPY_ENTROPY      phi = h                     dphi/dz_j = -(1 / ln c) p_j (log p_j + H)
 *   RTSDS_ENTROPY_ROBUST       phi = (h^2 + 1e-8)^eta      dphi/dz_j = 2 eta h (h^2 + 1e-8)^(eta - 1) * (the line above)
 *   RTSDS_ENTROPY_MAX_SQUARES  phi = -S / 2                dphi/dz_j = -p_j (p_j - S)
 * eta == 2 is formed as a product, any other eta with powf; eta is read only by ROBUST.  The
 * gradient term of a class with p_j == 0 is 0 under every penalty.  The probabilities never reach
 * memory.
 * rtsds_entropy_fwd: one launch, a workgroup per 128 consecutive pixels of the flattened [n h w]
 *   list, two adjacent lanes per pixel (even and odd classes; Z, H and S are the two lanes' sums
 *   added, a fixed order); workgroup i leaves (sum phi, sum h) of its tile in the workspace and, when want_grad, the
 *   fp32 term dphi/dz [n][h][w][c] behind the partials (want_grad == 0 writes none).  hmap (or NULL):
 *   fp32 [n][h][w] that receives h.
 * rtsds_entropy_finish: *loss = coef * sum phi, *mean_entropy = coef * sum h, both summed in a fixed
 *   order in fp64: the same bits on every run.  The caller passes coef = 1 / (n h w world).
 * rtsds_entropy_bwd: dx [n][h][w][c] (dtype) = cast(fp32(*grad_loss * coef_g) * term) from the term
 *   of a want_grad forward on the same workspace; coef_g = 1 / (n h w world).
 * None synchronises, allocates, clears memory, uses a float atomic or touches the host.  Before any
 * HIP call: RTSDS_ERR_SHAPE for a NULL tensor or scalar, a size < 1, c outside [2, 32], 2^31
 * elements or more, an unknown penalty, an eta or coefficient that is not finite (eta: and
 * positive); RTSDS_ERR_UNSUPPORTED for another dtype code, a tensor not aligned to its element, a
 * workspace not 16-B aligned; RTSDS_ERR_WORKSPACE for a NULL or short workspace
 * (rtsds_entropy_workspace bytes; 0 for a shape it refuses).                                       */
#define RTSDS_ENTROPY_ENTROPY 0
#define RTSDS_ENTROPY_ROBUST 1
#define RTSDS_ENTROPY_MAX_SQUARES 2
size_t rtsds_entropy_workspace(int n, int h, int w, int c);
int rtsds_entropy_fwd(const void* x, int dtype, int n, int h, int w, int c, int penalty, float eta, int want_grad, float* hmap,
                      void* wsp, size_t ws_bytes, void* stream);
int rtsds_entropy_finish(const void* wsp, size_t ws_bytes, int n, int h, int w, double coef, float* loss, float* mean_entropy,
                         void* stream);
int rtsds_entropy_bwd(const void* wsp, size_t ws_bytes, const float* grad_loss, double coef_g, void* dx, int dtype, int n, int h,
                      int w, int c, void* stream);

/* ---------------------------------------------------------------- graph replay
 * Replaces hipGraphLaunch of a captured multi-stream iteration (runtime.GraphedStep /
 * GraphedForward; the reference has no graphs: its train.py:65-113 / 172-284 loop bodies
 * launch every ATen kernel from the host).  rtsds_graph_split decomposes a captured hipGraph
 * (kernel / memcpy / memset / empty nodes) into at most max_lanes chains, cuts each chain at its
 * cross-chain edges into linear segments and instantiates one executable graph per segment;
 * rtsds_graph_split_launch replays them on one stream per chain (chain 0 = `stream`, which
 * also waits for the other chains at the end), with events for the cross-chain edges.  The
 * captured graph is only read (the caller keeps it and the memory it references alive).
 * Returns RTSDS_ERR_UNSUPPORTED for other node types (the caller replays the graph itself). */
int rtsds_graph_split(void* graph, int max_lanes, void** handle, int* n_segments, int* n_lanes);
/* Number of chains (<= max_lanes) rtsds_graph_split would use for `graph` -- 1 for a linear
 * (single-stream) capture; a negative RTSDS_ERR_* code on failure.  Nothing is instantiated. */
int rtsds_graph_lanes(void* graph, int max_lanes);
/* Number of nodes of a captured hipGraph (negative status on error); GraphedStep drops empty
 * segments (a capture between two back-to-back collectives). */
int rtsds_graph_nodes(void* graph);
/* Nodes captured so far by the capture `stream` records into (negative status when it is not
 * capturing); GraphedStep ends a graph segment at a collective only when it has nodes.        */
int rtsds_capture_nodes(void* stream);
int rtsds_graph_split_launch(void* handle, void* stream);
int rtsds_graph_split_destroy(void* handle);

/* Backward of the FFM attention on pooled vectors (build_bisenet.py:67-70): h = relu(conv1(p)),
 * a = sigmoid(conv2(h)), 1x1 convs on [n][c] rows (n <= 8, channels <= 64).  From da = dL/da:
 * dw2 / db2, dw1 / db1 (fp32 [cout][cin] / [cout]; overwritten, or added to when accumulate),
 * dp = dL/dp (stored).  w1 [c1][c0], w2 [c2][c1] in the compute dtype.  One launch; the
 * results equal the unfused chain's (act backward, pooled data / weight gradients) bit for bit
 * for channel counts that are not vector multiples (c % 8 bf16, c % 4 fp32).               */
int rtsds_pooled_mlp_bwd(const void* da, const void* a, const void* h, const void* p, const void* w1,
                         const void* w2, float* dw1, float* db1, float* dw2, float* db2, void* dp,
                         int n, int c0, int c1, int c2, int accumulate, int dtype, void* stream);

/* Its forward in one launch: h = relu(conv1(p) + b1), a = sigmoid(conv2(h) + b2) (b1 / b2 may
 * be NULL), h and a stored [n][c1] / [n][c2]; equal bit for bit to the two pooled 1x1 conv
 * launches of rtsds_conv2d_fwd for the same shapes (same limits as rtsds_pooled_mlp_bwd).     */
int rtsds_pooled_mlp_fwd(const void* p, const void* w1, const float* b1, const void* w2, const float* b2, void* h,
                         void* a, int n, int c0, int c1, int c2, int dtype, void* stream);

/* Training-mode tail of the FeatureFusionModule (build_bisenet.py:75-80) on a narrow class map
 * [n][hw][c] (c = 19, n <= 8, hw a multiple of the 16-B vector), in fewer launches than the
 * op-by-op chain and equal to it bit for bit (functional.FfmTailFn).
 *
 * rtsds_bn_fwd_gap: training BatchNorm + act of x (statistics / finalize as rtsds_bn_fwd, conv
 *   epilogue partials in stats_part / stats_nrb or NULL / 0), whose apply pass also leaves
 *   rtsds_gap_fwd's stage-1 partials of y in gap_part (rtsds_gap_workspace(n, hw, c) bytes).
 * rtsds_ffm_att_scale: from those partials pooled = GAP(f), hid = relu(conv1(pooled) + b1),
 *   att = sigmoid(conv2(hid) + b2) (each [n][c]) and r = f * att + f, one launch.  r has pixel
 *   pitch ldr: c, or a vector multiple up to 64 with zeros beyond c (RTSDS_INPUT_PADDED's form).
 * rtsds_ffm_att_bwd: from dr = dL/dr the attention's whole backward (rtsds_chscale_bwd's da, then
 *   rtsds_pooled_mlp_bwd) in two launches; ws: rtsds_gap_workspace(n, hw, c) bytes.
 * rtsds_bn_bwd_ffm: rtsds_bn_bwd of that BatchNorm with its incoming gradient
 *   round(round(dr * (att + 1)) + round(dpooled / hw)) formed per element instead of stored
 *   (rtsds_chscale_bwd's dx followed by rtsds_gap_bwd's accumulate).                            */
int rtsds_bn_fwd_gap(const void* x, void* y, float* gap_part, int n, long hw, int c, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, long long* num_batches_tracked, float* save_mean,
                     float* save_invstd, float momentum, float eps, int act, const float* stats_part, int stats_nrb,
                     int dtype, void* ws, size_t ws_bytes, void* stream);
int rtsds_ffm_att_scale(const float* part, const void* f, const void* w1, const float* b1, const void* w2, const float* b2,
                        void* pooled, void* hid, void* att, void* r, int ldr, int n, long hw, int c, int dtype,
                        void* stream);
int rtsds_ffm_att_bwd(const void* dr, const void* f, const void* a, const void* h, const void* p, const void* w1,
                      const void* w2, float* dw1, float* db1, float* dw2, float* db2, void* dp, int n, long hw, int c,
                      int accumulate, int dtype, void* ws, size_t ws_bytes, void* stream);
int rtsds_bn_bwd_ffm(const void* dr, const void* att, const void* dpooled, int n, long hw, const void* x, void* dx,
                     float* dgamma, float* dbeta, int c, const float* gamma, const float* beta, const float* save_mean,
                     const float* save_invstd, int training, int act, int accumulate_params, int dtype, void* ws,
                     size_t ws_bytes, void* stream);

/* Label statistics for class weighting (csrc/labelstat.hip).  label: int64 [n][h][w]; per call
 * count[k] += pixels labelled k and support[k] += valid pixels (label in [0, c)) of the images of
 * this batch that contain class k, k < c <= 32; a label equal to ignore_index or outside [0, c)
 * enters neither.  count / support: c uint64 each, accumulated into (the caller zeroes them once).
 * Integers only: exact, order-independent; no host sync, no memset (graph-capture safe).
 * RTSDS_ERR_SHAPE: a NULL label / count / support, n outside [1, 65535], h or w < 1, h * w above
 * 2^32 - 1, c outside [1, 32]; RTSDS_ERR_WORKSPACE: a NULL or short ws (the query returns 0 for a
 * shape it refuses); all before any launch.                                                   */
size_t rtsds_label_stats_workspace(int n, int c);
int rtsds_label_stats(const int64_t* label, int n, int h, int w, int c, int ignore_index,
                      unsigned long long* count, unsigned long long* support, void* ws, size_t ws_bytes,
                      void* stream);

/* ABI revision of this header (RTSDS_ABI_VERSION): bumped whenever an entry point's signature
 * changes.  The Python loader refuses a library whose revision differs (A/B variant libraries
 * built from older sources would otherwise be called with the wrong argument lists). */
#define RTSDS_ABI_VERSION 29
int rtsds_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* RTSDS_HIP_H */
