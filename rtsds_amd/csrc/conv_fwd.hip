// Convolution forward, host side (C ABI): the route of a descriptor -- a direct kernel (pooled /
// tapconv / hconv / imgconv) or the implicit GEMM (conv_gemm_kernel.h, instantiated in
// conv_gemm_fwd.hip) -- the workspace plan, and the operand kernels of the GEMM route: channel
// padding, the superpixel image view, the split-K reduce.
#include "conv_host.h"

// dst[r][j] = j < c ? src[r][j] : 0   (channel padding of an NHWC tensor or of [co][tap][ci] weights)
// One thread per 16-byte output vector: dst[r][j0..j0+V) = src[r][j] (j < c) or 0.
template <typename T>
__global__ void __launch_bounds__(256) pad_channels_kernel(const T* __restrict__ src, T* __restrict__ dst, int total, int c,
                                                            int cpv, FastDiv fcpv) {
  constexpr int V = VecT<T>::N;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int r = (int)fdiv((uint32_t)i, fcpv);
    const int j0 = (i - r * cpv) * V;
    const T* s = src + (long)r * c;
    typename VecT<T>::v16 o;
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = j0 + e < c ? s[j0 + e] : (T)0.0f;
    *(typename VecT<T>::v16*)(dst + (long)i * V) = o;
  }
}

template <typename T>
static void pad_launch(const void* src, void* dst, long rows, int c, int cp, hipStream_t st) {
  const int cpv = cp / VecT<T>::N;
  const long total = rows * cpv;  // < 2^31 (checked by check_desc via the element count)
  const int blocks = (int)std::max<long>(1, std::min<long>(1 << 16, (total + 255) / 256));
  hipLaunchKernelGGL(pad_channels_kernel<T>, dim3(blocks), dim3(256), 0, st, (const T*)src, (T*)dst, (int)total, c, cpv,
                     fastdiv_make(cpv));
}
int pad_any(int dtype, const void* src, void* dst, long rows, int c, int cp, hipStream_t st) {
  DISPATCH_T(dtype, pad_launch<T>(src, dst, rows, c, cp, st));
  return RTSDS_OK;
}

__global__ void __launch_bounds__(256) sp_pad4_kernel(const bf16* __restrict__ x, bf16* __restrict__ x4, long pixels) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= pixels) return;
  bf16x4 v;
  v[0] = x[i * 3];
  v[1] = x[i * 3 + 1];
  v[2] = x[i * 3 + 2];
  v[3] = (bf16)0.f;
  *(bf16x4*)(x4 + i * 4) = v;
}
// w[k][r][s][3] -> w'[k][r][p][q*4 + ch], s = 2p - 1 + q (zero outside [0, kw), ch == 3).
__global__ void __launch_bounds__(256) sp_repack_w_kernel(const bf16* __restrict__ w, bf16* __restrict__ wp, int k, int kh,
                                                          int kw, int kwp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= k * kh * kwp * 8) return;
  const int e = i & 7, t = i >> 3;
  const int p = t % kwp, kr = t / kwp;  // kr = co * kh + r
  const int s = 2 * p - 1 + (e >> 2), ch = e & 3;
  wp[i] = (s >= 0 && s < kw && ch < 3) ? w[((long)kr * kw + s) * 3 + ch] : (bf16)0.f;
}
void sp_pad4(const rtsds_conv_desc* d, const void* x, void* x4, hipStream_t st) {
  const long px = (long)d->n * d->h * d->w;
  hipLaunchKernelGGL(sp_pad4_kernel, dim3((unsigned)((px + 255) / 256)), dim3(256), 0, st, (const bf16*)x, (bf16*)x4, px);
}

// The forward route of a descriptor: a direct kernel where one applies, else the implicit GEMM.
// accum: y += result (the plain forward's RTSDS_ACCUMULATE); res: a residual operand (the
// BatchNorm-folded forward).  The one ladder behind the statistics-tile count and every entry.
enum FwdRoute { FWD_POOLED, FWD_TAP, FWD_HALO, FWD_IMG, FWD_GEMM };
static FwdRoute fwd_route(const rtsds_conv_desc* d, bool accum = false, bool res = false) {
  if (pooled_1x1(d) && !res) return FWD_POOLED;
  if (tapconv_ok(d) && !accum) return FWD_TAP;
  if (hconv_ok(d) && !accum) return FWD_HALO;
  if (imgconv_ok(d) && !accum && !res) return FWD_IMG;
  return FWD_GEMM;
}

// Number of M tiles (= BatchNorm partial-statistics rows) the forward launch of d uses.
extern "C" int rtsds_conv2d_fwd_stats_tiles(const rtsds_conv_desc* d) {
  switch (fwd_route(d)) {
    case FWD_POOLED: return 1;
    case FWD_TAP: return tapconv_rows(d, 0);
    case FWD_HALO: return hconv_tiles(d);
    case FWD_IMG: return imgconv_tiles(d);
    case FWD_GEMM: break;
  }
  int bm, bn;
  const long M = (long)d->n * d->ho * d->wo;
  const long K = sp_path(d) ? 0 : (long)d->kh * d->kw * pad_c(d->c, d->dtype);  // rtsds_conv2d_fwd's p.K
  pick_tile(M, d->k, d->dtype == RTSDS_BF16, bm, bn, true, K);
  return (int)((M + bm - 1) / bm);
}

// Channel pitch of x the forward / weight-gradient gathers read (RTSDS_INPUT_PADDED: the caller
// hands x with this pitch, zero beyond c): 4 for the superpixel image convs, the vector-padded
// channel count for the implicit GEMM, c itself for the pooled and halo paths.
static int input_pitch(const rtsds_conv_desc* d) {
  if (pooled_1x1(d) || hconv_ok(d)) return d->c;
  if (sp_path(d)) return 4;
  return pad_c(d->c, d->dtype);
}
extern "C" int rtsds_conv2d_input_pitch(const rtsds_conv_desc* d) {
  return check_desc(d) ? 0 : input_pitch(d);
}

// FWD split-K for narrow outputs (<= 32 channels: DeepLab's ASPP branches, 2048 -> 19 classes
// at 65x129, K = 18,432): the 128x32 tiles of M = 33,540 rows make 263 workgroups, one 4-wave
// group per CU walking 288 K-tiles, latency-bound on the operand gathers.  S K-splits (>= 16
// K-tiles each) into fp32 slabs [S][M][N] put ~6 groups on every CU (194 -> 100 us); fwd_split_reduce_kernel
// sums them in split order and adds the bias (and y, for ConvSum's accumulate).  Only without
// BatchNorm-statistics / activation epilogues; BK = 64 (LDS-DMA path: Cin % 32 == 0).
struct FwdSplit {
  int splits, tps;
  size_t slab_bytes;
};
static FwdSplit fwd_split(const rtsds_conv_desc* d) {
  FwdSplit s = {1, 1 << 30, 0};
  if (d->dtype != RTSDS_BF16 || d->k > 32 || d->c % 32 != 0 || pooled_1x1(d) || hconv_ok(d) || sp_path(d)) return s;
  const long M = (long)d->n * d->ho * d->wo;
  const int nk = (d->kh * d->kw * d->c + 63) / 64;
  int bm, bn;
  pick_tile(M, d->k, true, bm, bn, true);
  const long tiles = (M + bm - 1) / bm;
  if (tiles >= 512 || nk < 32) return s;
  const int want = (int)std::min<long>((1536 + tiles - 1) / tiles, nk / 16);
  if (want < 2) return s;
  s.tps = (nk + want - 1) / want;
  s.splits = (nk + s.tps - 1) / s.tps;
  s.slab_bytes = al256((size_t)s.splits * M * d->k * 4);
  return s;
}

// y (+)= bias + sum_s slab[s] -> bf16, the split order fixed (deterministic)
__global__ void __launch_bounds__(256) fwd_split_reduce_kernel(const float* __restrict__ slab, const float* __restrict__ bias,
                                                               bf16* __restrict__ y, long total, int n, long stride,
                                                               int splits, int accum) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    float s = slab[i];
    for (int q = 1; q < splits; ++q) s += slab[q * stride + i];
    if (bias) s += bias[i % n];
    if (accum) s += to_f(y[i]);
    y[i] = from_f<bf16>(s);
  }
}

// FWD workspace, one plan for the query and the launches: [x copy][w copy][split-K slabs].  The
// operand copies are the superpixel view of the 3-channel stride-2 convs (x padded to 4 channels,
// w repacked) or channel-padded copies when Cin is not a vector multiple; g is the conv the GEMM
// then runs.  (RTSDS_INPUT_PADDED leaves the x region unused, not smaller; the direct image conv
// uses the x region only.)
struct FwdPlan {
  rtsds_conv_desc g;
  bool sp;
  size_t x_bytes, w_bytes;
  FwdSplit split;
  size_t total() const { return x_bytes + w_bytes + split.slab_bytes; }
  void* x(void* ws) const { return ws; }
  void* w(void* ws) const { return (char*)ws + x_bytes; }
  float* slab(void* ws) const { return (float*)((char*)ws + x_bytes + w_bytes); }
};
static FwdPlan fwd_plan(const rtsds_conv_desc* d) {
  FwdPlan pl = {*d, false, 0, 0, fwd_split(d)};
  if (pooled_1x1(d) || hconv_ok(d)) return pl;
  if (sp_path(d)) {
    pl.sp = true;
    pl.g = sp_desc(d);
    pl.x_bytes = sp_x4_bytes(d);
    pl.w_bytes = sp_w_bytes(d);
    return pl;
  }
  const int cp = pad_c(d->c, d->dtype);
  if (cp != d->c) {
    const size_t es = esize(d->dtype);
    pl.x_bytes = al256((size_t)d->n * d->h * d->w * cp * es);
    pl.w_bytes = al256((size_t)d->k * d->kh * d->kw * cp * es);
    pl.g.c = cp;
  }
  return pl;
}
extern "C" size_t rtsds_conv2d_fwd_workspace(const rtsds_conv_desc* d) { return fwd_plan(d).total(); }

// What the three forward entries hand to a route: the epilogue operands (ConvArgs names them).
struct FwdEpi {
  const float* bias;   // or the folded BatchNorm's shift
  const float* scale;  // the folded BatchNorm's scale (or null)
  const void* res;
  void* y;
  int act, accum;
  float* stats;
  int ldo;
};

// The implicit-GEMM route: the plan's operand copies, ConvArgs, the launch.
static int fwd_gemm(const rtsds_conv_desc* d0, const FwdPlan& pl, const void* x, const void* w, const FwdEpi& e, bool x_padded,
                    void* ws, hipStream_t st) {
  const rtsds_conv_desc& d = pl.g;
  // the gathers read 16-B vectors of Cin: a descriptor whose plan reserves no padded copy (a
  // pooled vector with a residual) has no route here unless Cin already is a vector multiple
  if (d.c % (16 / (int)esize(d.dtype)) != 0) return RTSDS_ERR_UNSUPPORTED;
  if (pl.sp) {
    if (!x_padded) sp_pad4(d0, x, pl.x(ws), st);
    const int n = d0->k * d0->kh * d.kw * 8;
    hipLaunchKernelGGL(sp_repack_w_kernel, dim3(rt_cdiv(n, 256)), dim3(256), 0, st, (const bf16*)w, (bf16*)pl.w(ws), d0->k,
                       d0->kh, d0->kw, d.kw);
  } else if (pl.w_bytes) {
    int err = x_padded ? RTSDS_OK : pad_any(d.dtype, x, pl.x(ws), (long)d.n * d.h * d.w, d0->c, d.c, st);
    if (!err) err = pad_any(d.dtype, w, pl.w(ws), (long)d.k * d.kh * d.kw, d0->c, d.c, st);
    if (err) return err;
  }
  if (pl.w_bytes) {
    if (!x_padded) x = pl.x(ws);
    w = pl.w(ws);
  }
  ConvArgs p = make_args(&d);
  p.a = x; p.b = w; p.bias = e.bias; p.scale = e.scale; p.res = e.res; p.out = e.y;
  p.act = e.act;
  p.accum = e.accum;
  p.stats = e.stats;
  p.ldo = e.ldo;
  p.M = d.n * d.ho * d.wo;
  p.N = d.k;
  p.K = d.kh * d.kw * d.c;
  // split-K only under the plain epilogue (bias, accumulate): the reduce applies nothing else
  if (pl.split.splits > 1 && !e.stats && e.act == 0 && !e.scale) {
    p.slab = pl.slab(ws);
    p.tiles_per_split = pl.split.tps;
    p.split_stride = (long)p.M * p.N;
    dispatch_align<bf16, MODE_FWD>(p, d.c, st, pl.split.splits);
    const long total = (long)p.M * p.N;
    hipLaunchKernelGGL(fwd_split_reduce_kernel, dim3((int)std::min<long>(8192, (total + 255) / 256)), dim3(256), 0, st,
                       (const float*)p.slab, e.bias, (bf16*)e.y, total, p.N, p.split_stride, pl.split.splits, p.accum);
    RET_LAUNCH();
  }
  DISPATCH_T(d.dtype, dispatch_align<T, MODE_FWD>(p, d.c, st));
  RET_LAUNCH();
}

static int fwd_launch(FwdRoute route, const rtsds_conv_desc* d0, const FwdPlan& pl, const void* x, const void* w, const FwdEpi& e,
                      bool x_padded, void* ws, hipStream_t st) {
  switch (route) {
    case FWD_POOLED: return pooled_fwd(d0, x, w, e.bias, e.y, e.act, e.accum, e.stats, e.scale, st);
    case FWD_TAP: tapconv_fwd(d0, x, w, e.bias, e.scale, e.res, e.y, e.act, e.stats, st); break;
    case FWD_HALO: hconv_fwd(d0, x, w, e.bias, e.scale, e.res, e.y, e.act, e.stats, st); break;
    case FWD_IMG:
      if (!x_padded) sp_pad4(d0, x, pl.x(ws), st);
      imgconv_fwd(d0, x_padded ? x : pl.x(ws), w, e.bias, e.scale, e.y, e.act, e.stats, st);
      break;
    case FWD_GEMM: return fwd_gemm(d0, pl, x, w, e, x_padded, ws, st);
  }
  RET_LAUNCH();
}

extern "C" int rtsds_conv2d_fwd(const rtsds_conv_desc* d0, const void* x, const void* w, const float* bias,
                                void* y, int act, float* bn_stats, void* ws, size_t ws_bytes, void* stream) {
  int e = check_desc(d0);
  if (e) return e;
  const FwdPlan pl = fwd_plan(d0);
  if (ws_bytes < pl.total()) return RTSDS_ERR_WORKSPACE;
  const FwdEpi ep = {bias, nullptr, nullptr, y, act & 0xff, (act & RTSDS_ACCUMULATE) ? 1 : 0, bn_stats, 0};
  // (the statistics come from the conv's exact values: no epilogue may follow them, on any route)
  if (bn_stats && (ep.act || ep.accum)) return RTSDS_ERR_UNSUPPORTED;
  const FwdRoute route = fwd_route(d0, ep.accum != 0);
  const bool x_padded = (act & RTSDS_INPUT_PADDED) != 0;  // (nothing to pad in a pooled vector: ignored there)
  if (route != FWD_POOLED && x_padded && input_pitch(d0) == d0->c) return RTSDS_ERR_UNSUPPORTED;
  return fwd_launch(route, d0, pl, x, w, ep, x_padded, ws, (hipStream_t)stream);
}

// Eval-mode conv + BatchNorm(running statistics) [+ residual] [+ activation] in one launch:
// y = act(conv(x, w) * scale + shift + res), scale / shift from rtsds_bn_fold.
extern "C" int rtsds_conv2d_fwd_bn(const rtsds_conv_desc* d0, const void* x, const void* w, const float* scale,
                                   const float* shift, const void* res, void* y, int act, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (!scale || !shift || (act & RTSDS_ACCUMULATE)) return RTSDS_ERR_UNSUPPORTED;
  int e = check_desc(d0);
  if (e) return e;
  const FwdPlan pl = fwd_plan(d0);
  if (ws_bytes < pl.total()) return RTSDS_ERR_WORKSPACE;
  const bool x_padded = (act & RTSDS_INPUT_PADDED) != 0;
  if (x_padded && input_pitch(d0) == d0->c) return RTSDS_ERR_UNSUPPORTED;
  const FwdEpi ep = {shift, scale, res, y, act & 0xff, 0, nullptr, 0};
  return fwd_launch(fwd_route(d0, false, res != nullptr), d0, pl, x, w, ep, x_padded, ws, (hipStream_t)stream);
}

extern "C" int rtsds_conv2d_fwd_bn_ld(const rtsds_conv_desc* d0, const void* x, const void* w, const float* scale,
                                      const float* shift, void* y, long ldy, int act, void* ws, size_t ws_bytes,
                                      void* stream) {
  if (!scale || !shift || (act & RTSDS_ACCUMULATE)) return RTSDS_ERR_UNSUPPORTED;
  int e = check_desc(d0);
  if (e) return e;
  if (ldy == d0->k) return rtsds_conv2d_fwd_bn(d0, x, w, scale, shift, nullptr, y, act, ws, ws_bytes, stream);
  // a channel slice of a wider NHWC tensor: the implicit-GEMM route with 16-B row chunks only
  const int vec = 16 / esize(d0->dtype);
  if (ldy < d0->k || ldy % vec || d0->k % vec || ((uintptr_t)y & 15) || ldy > (1L << 30)) return RTSDS_ERR_UNSUPPORTED;
  if (fwd_route(d0) != FWD_GEMM) return RTSDS_ERR_UNSUPPORTED;
  const FwdPlan pl = fwd_plan(d0);
  if (ws_bytes < pl.total()) return RTSDS_ERR_WORKSPACE;
  const bool x_padded = (act & RTSDS_INPUT_PADDED) != 0;
  if (x_padded && input_pitch(d0) == d0->c) return RTSDS_ERR_UNSUPPORTED;
  const FwdEpi ep = {shift, scale, nullptr, y, act & 0xff, 0, nullptr, (int)ldy};
  return fwd_launch(FWD_GEMM, d0, pl, x, w, ep, x_padded, ws, (hipStream_t)stream);
}

extern "C" int rtsds_conv2d_fwd_bn_maxpool(const rtsds_conv_desc* d0, const void* x, const void* w, const float* scale,
                                           const float* shift, void* y, int act, int hp, int wp, int pool_pad, void* ws,
                                           size_t ws_bytes, void* stream) {
  if (!scale || !shift || (act & RTSDS_ACCUMULATE)) return RTSDS_ERR_UNSUPPORTED;
  int e = check_desc(d0);
  if (e) return e;
  if (!imgconv_pool_ok(d0, hp, wp) || pool_pad < 0 || pool_pad > 1) return RTSDS_ERR_UNSUPPORTED;
  // the windows must cover the pooled grid: hp <= ceil((ho + 2 pad - 3) / 2) + 1
  if (hp > (d0->ho + 2 * pool_pad - 3 + 1) / 2 + 1 || wp > (d0->wo + 2 * pool_pad - 3 + 1) / 2 + 1) return RTSDS_ERR_SHAPE;
  const FwdPlan pl = fwd_plan(d0);
  if (ws_bytes < pl.total()) return RTSDS_ERR_WORKSPACE;
  const bool x_padded = (act & RTSDS_INPUT_PADDED) != 0;
  hipStream_t st = (hipStream_t)stream;
  if (!x_padded) sp_pad4(d0, x, pl.x(ws), st);
  imgconv_pool_fwd(d0, x_padded ? x : pl.x(ws), w, shift, scale, y, act & 0xff, hp, wp, pool_pad, st);
  RET_LAUNCH();
}
