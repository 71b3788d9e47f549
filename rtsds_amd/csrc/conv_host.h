// Convolution host side, shared by the three pass units (conv_{fwd,dgrad,wgrad}.hip), the pooled
// unit (conv_pooled.hip) and the direct-kernel units (hconv / tapconv / imgconv / pw): descriptor
// checks, channel padding, the implicit GEMM's arguments, the route predicates that need no
// kernel, and -- declared once -- every entry point one conv unit calls in another, so a
// definition is checked against the declaration its callers see.
#pragma once
#include "conv_args.h"
#include <algorithm>

static inline size_t esize(int dtype) { return dtype == RTSDS_BF16 ? 2 : 4; }
static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

static inline int check_desc(const rtsds_conv_desc* d) {
  if (d->n <= 0 || d->h <= 0 || d->w <= 0 || d->c <= 0 || d->k <= 0 || d->kh <= 0 || d->kw <= 0 ||
      d->sh <= 0 || d->sw <= 0 || d->dh <= 0 || d->dw <= 0 || d->ph < 0 || d->pw < 0)
    return RTSDS_ERR_SHAPE;
  const int ho = (d->h + 2 * d->ph - d->dh * (d->kh - 1) - 1) / d->sh + 1;
  const int wo = (d->w + 2 * d->pw - d->dw * (d->kw - 1) - 1) / d->sw + 1;
  if (ho != d->ho || wo != d->wo || ho <= 0 || wo <= 0) return RTSDS_ERR_SHAPE;
  if (d->dtype != RTSDS_F32 && d->dtype != RTSDS_BF16) return RTSDS_ERR_UNSUPPORTED;
  if ((long)d->n * d->h * d->w * 32 * ((d->c + 31) / 32) >= (1L << 31) ||
      (long)d->n * d->ho * d->wo * 32 * ((d->k + 31) / 32) >= (1L << 31))
    return RTSDS_ERR_UNSUPPORTED;
  return RTSDS_OK;
}

// Channel padding target so every gather runs on 16-B vectors: channel counts that are not a
// multiple of the vector width (3-channel images, 19-class maps, the 1-channel D logit) are
// zero-padded into workspace -- to a multiple of 32 (one filter tap per K-tile) when that
// costs < 1.7x, else to the vector width.
static inline int pad_c(int c, int dtype) {
  const int V = dtype == RTSDS_BF16 ? 8 : 4;
  if (c % V == 0) return c;
  const int c32 = (c + 31) / 32 * 32;
  if (c >= 8 && c32 * 10 < c * 17) return c32;
  return (c + V - 1) / V * V;
}

static inline ConvArgs make_args(const rtsds_conv_desc* d) {
  ConvArgs p = {};
  p.n = d->n; p.h = d->h; p.w = d->w; p.c = d->c; p.ho = d->ho; p.wo = d->wo; p.k = d->k;
  p.kh = d->kh; p.kw = d->kw; p.sh = d->sh; p.sw = d->sw; p.ph = d->ph; p.pw = d->pw;
  p.dh = d->dh; p.dw = d->dw;
  p.f_howo = fastdiv_make(d->ho * d->wo);
  p.f_wo = fastdiv_make(d->wo);
  p.f_hw = fastdiv_make(d->h * d->w);
  p.f_w = fastdiv_make(d->w);
  p.f_c = fastdiv_make(d->c);
  p.f_k = fastdiv_make(d->k);
  p.f_kw = fastdiv_make(d->kw);
  p.tkw = d->kw; p.f_tkw = p.f_kw;
  p.r0h = p.r0w = 0; p.rstep = 1; p.psh = 1; p.offh = p.offw = 0;
  p.hp = d->h; p.wp = d->w;
  p.tiles_per_split = 1 << 30;
  const int hw = d->ho * d->wo;
  p.wg_rows = (hw % 64 == 0) && (d->wo % 64 == 0 || 64 % d->wo == 0);
  const long big = std::max((long)d->n * d->h * d->w * d->c, (long)d->n * d->ho * d->wo * d->k) * (long)esize(d->dtype);
  p.gbuf = big < (1L << 31) && (long)d->k * d->kh * d->kw * d->c * (long)esize(d->dtype) < (1L << 31);
  return p;
}

// ---- pooled-vector 1x1 convs (ARM / FFM attention on [N, C, 1, 1], build_bisenet.py:41,
// 67-69): M = N <= 32 rows, a GEMV-sized problem.  One launch per pass, no channel padding,
// fp32 accumulation, BatchNorm partial statistics (one "tile" of M rows) from the exact values.
// (conv_pooled.hip; each launch ends the entry point: it returns the launch status.)
static const int kPooledMaxRows = 32;
static inline bool pooled_1x1(const rtsds_conv_desc* d) {
  return d->h == 1 && d->w == 1 && d->kh == 1 && d->kw == 1 && d->sh == 1 && d->sw == 1 && d->ph == 0 &&
         d->pw == 0 && d->n <= kPooledMaxRows;
}
int pooled_fwd(const rtsds_conv_desc* d, const void* x, const void* w, const float* bias, void* y, int act, int accum,
               float* stats, const float* scale, hipStream_t st);
int pooled_dgrad(const rtsds_conv_desc* d, const void* dy, const void* w, void* dx, int accum, hipStream_t st);
int pooled_wgrad(const rtsds_conv_desc* d, const void* x, const void* dy, float* dw, float* dbias, int accum, hipStream_t st);

// ---- 3-channel stride-2 convs on the image (ResNet stem 7x7 s2 p3, build_contextpath.py via
// torchvision conv1; spatial-path ConvBlock 3x3 s2 p1, build_bisenet.py:9-14).  Gathering one
// 16-B chunk per tap would carry 3 useful channels of 8 (and 8/3 of the MFMA K): instead the
// image is padded to 4 channels and viewed as "superpixels" of two horizontally adjacent
// pixels (8 bf16 = one 16-B chunk).  With odd padding pw, taps s = 2p - 1 + q (q = 0, 1) of
// output column ow read superpixel ow - (pw + 1) / 2 + p, so the conv becomes an ordinary
// implicit GEMM over (row tap, tap pair, 8 elements) with stride (2, 1): K = kh * (kw + 1) / 2 * 8
// (stem: 224 instead of 392), every chunk 16-B aligned and fully in or out of the padding.
static inline bool sp_path(const rtsds_conv_desc* d) {
  return d->dtype == RTSDS_BF16 && d->c == 3 && d->sh == 2 && d->sw == 2 && d->dh == 1 && d->dw == 1 &&
         (d->pw & 1) == 1 && (d->kw & 1) == 1 && (d->w & 1) == 0;
}
static inline rtsds_conv_desc sp_desc(const rtsds_conv_desc* d) {
  rtsds_conv_desc v = *d;
  v.w = d->w / 2;
  v.c = 8;
  v.kw = (d->kw + 1) / 2;
  v.sw = 1;
  v.pw = (d->pw + 1) / 2;
  return v;
}
static inline size_t sp_x4_bytes(const rtsds_conv_desc* d) { return ((size_t)d->n * d->h * d->w * 8 + 255) & ~(size_t)255; }
static inline size_t sp_w_bytes(const rtsds_conv_desc* d) {
  return ((size_t)d->k * d->kh * ((d->kw + 1) / 2) * 16 + 255) & ~(size_t)255;
}

// Operand copies, defined in conv_fwd.hip and used by all three passes (no kernel template is
// instantiated from two units): dst[r][0..cp) = src[r][0..c) then zeros; the 3 -> 4 channel
// image pad of the superpixel view.
int pad_any(int dtype, const void* src, void* dst, long rows, int c, int cp, hipStream_t st);
void sp_pad4(const rtsds_conv_desc* d, const void* x, void* x4, hipStream_t st);

// Halo-resident direct conv for narrow 3x3 outputs (hconv.hip).
bool hconv_ok(const rtsds_conv_desc* d);
int hconv_tiles(const rtsds_conv_desc* d);
void hconv_fwd(const rtsds_conv_desc* d, const void* x, const void* w, const float* bias, const float* scale, const void* res, void* y,
               int act, float* stats, hipStream_t st);
bool hconv_dgrad_ok(const rtsds_conv_desc* d);
bool nwgrad_ok(const rtsds_conv_desc* d);
int nwgrad_splits(const rtsds_conv_desc* d);
void nwgrad(const rtsds_conv_desc* d, const void* x, const void* dyp, float* slab, hipStream_t st);
void hconv_dgrad(const rtsds_conv_desc* d, const void* dyp, int kp, const void* wt, void* dx, int accumulate, hipStream_t st);
// Direct FMA data gradient of the narrow-output 1x1 convs (pw.hip).
bool pw_ok(const rtsds_conv_desc* d);
void pw_dgrad(const rtsds_conv_desc* d, const void* dy, const void* w, void* dx, int accum, hipStream_t st);
// Direct MFMA conv for the 3-channel stride-2 image convs (imgconv.hip).
bool imgconv_ok(const rtsds_conv_desc* d);
bool imgconv_pool_ok(const rtsds_conv_desc* d, int hp, int wp);
void imgconv_pool_fwd(const rtsds_conv_desc* d, const void* x4, const void* w, const float* shift, const float* scale, void* y,
                      int act, int hp, int wp, int pp, hipStream_t st);
int imgconv_tiles(const rtsds_conv_desc* d);
void imgconv_fwd(const rtsds_conv_desc* d, const void* x4, const void* w, const float* bias, const float* scale, void* y,
                 int act, float* stats, hipStream_t st);
// Register-resident-weight direct conv for 3x3 64 -> 64 stride-1 convs (tapconv.hip).
bool tapconv_ok(const rtsds_conv_desc* d);
int tapconv_rows(const rtsds_conv_desc* d, int dgrad);
void tapconv_fwd(const rtsds_conv_desc* d, const void* x, const void* w, const float* bias, const float* scale, const void* res,
                 void* y, int act, float* stats, hipStream_t st);
void tapconv_dgrad(const rtsds_conv_desc* d, const void* dy, const void* wt, void* dx, int accumulate, const void* mask,
                   int mask_act, float* bnb_part, const void* bnb_x, const float* gamma, const float* beta, const float* mean,
                   const float* invstd, int bnb_act, hipStream_t st);
