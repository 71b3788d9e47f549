// Convolution data gradient, host side (C ABI): the route of a descriptor -- a direct kernel
// (pooled / pw / tapconv / hconv) or the implicit GEMM (conv_gemm_kernel.h, instantiated in
// conv_gemm_dgrad.hip), at stride 2 as parity phases -- the workspace plan, the weight pre-pack,
// and the helper kernels: weight repacks, the split-K reduce.
#include "conv_host.h"

// W[co][r][s][ci] -> Wt[ci][rr][ss][co_p] (DGRAD's B operand) over the taps
// r = r0h + rr*rstep (rr < tkh), s = r0w + ss*rstep (ss < tkw); zero for co >= co_n.
template <typename T>
__global__ void repack_wt_kernel(const T* __restrict__ w, T* __restrict__ wt, int co_n, int co_p, int kh, int kw, int ci_n,
                                 int tkh, int tkw, int r0h, int r0w, int rstep) {
  const int taps = tkh * tkw;
  const long total = (long)co_p * taps * ci_n;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int co = (int)(i % co_p);
    const long rest = i / co_p;
    const int tap = (int)(rest % taps);
    const int ci = (int)(rest / taps);
    const int r = r0h + (tap / tkw) * rstep, sc = r0w + (tap % tkw) * rstep;
    wt[i] = co < co_n ? w[(((long)co * kh + r) * kw + sc) * ci_n + ci] : (T)0.0f;
  }
}

// All stride-2 DGRAD phases in one launch (blockIdx.y = phase): Wt_phase[ci][tap][co_p] at
// element offset boff[phase] (32-bit indexing: a conv's weights are far below 2^31 elements).
struct RepackPhases {
  int tkh[4], tkw[4], r0h[4], r0w[4];
  long boff[4];
};
template <typename T>
__global__ void __launch_bounds__(256) repack_phases_kernel(const T* __restrict__ w, T* __restrict__ wt, int co_n, int co_p, int kh,
                                                            int kw, int ci_n, int rstep, RepackPhases rp) {
  const int ph = blockIdx.y;
  const int tkw = rp.tkw[ph], taps = rp.tkh[ph] * tkw;
  const int total = co_p * taps * ci_n;
  T* out = wt + rp.boff[ph];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int co = i % co_p, rest = i / co_p;
    const int tap = rest % taps, ci = rest / taps;
    const int r = rp.r0h[ph] + (tap / tkw) * rstep, sc = rp.r0w[ph] + (tap % tkw) * rstep;
    out[i] = co < co_n ? w[((co * kh + r) * kw + sc) * ci_n + ci] : (T)0.0f;
  }
}

// DGRAD split-K for small-M deep stride-1 convs (ResNet layer4: M = 4096 pixels, K = 4608):
// the occupancy rule would fall back to 64x64 tiles (AI 32 flop/B of staged operands); 128x128
// tiles x S K-splits keep the MFMA-dense tile and still put >= 512 workgroups on the chip.
// fp32 slabs [S][M][N] summed in split order (+ accumulate) into the bf16 dx.
struct DgradSplit {
  int splits, tps;
  size_t slab_bytes;
};
static DgradSplit dgrad_split(const rtsds_conv_desc* d, int kp) {
  DgradSplit s = {1, 1 << 30, 0};
  if (d->dtype != RTSDS_BF16 || d->sh != 1 || d->sw != 1 || kp % 64 != 0 || d->c % 8 != 0) return s;
  const long M = (long)d->n * d->h * d->w;
  const int N = d->c, K = d->kh * d->kw * kp;
  int bm, bn;
  pick_tile(M, N, true, bm, bn);
  if (!(bm == 64 && bn == 64)) return s;  // the wide tiles already fill the chip
  const long tiles = ((M + 127) / 128) * ((N + 127) / 128);
  const int nk = (K + 63) / 64;
  int want = (int)std::min<long>(8, (512 + tiles - 1) / tiles);
  want = std::min(want, nk / 16);  // >= 16 K-tiles per split
  if (want < 2) return s;
  s.tps = (nk + want - 1) / want;
  s.splits = (nk + s.tps - 1) / s.tps;
  s.slab_bytes = al256((size_t)s.splits * M * N * 4);
  return s;
}
// dx (+)= sum_s slab[s] -> bf16; 8 channels per thread
__global__ void __launch_bounds__(256) dgrad_split_reduce_kernel(const float* __restrict__ slab, bf16* __restrict__ dx, long nv8,
                                                                long stride, int splits, int accum) {
  for (long i = blockIdx.x * 256L + threadIdx.x; i < nv8; i += (long)gridDim.x * 256) {
    float s[8];
    {
      const f32x4 a = *(const f32x4*)(slab + i * 8), b = *(const f32x4*)(slab + i * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { s[e] = a[e]; s[4 + e] = b[e]; }
    }
    for (int q = 1; q < splits; ++q) {
      const f32x4 a = *(const f32x4*)(slab + q * stride + i * 8), b = *(const f32x4*)(slab + q * stride + i * 8 + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) { s[e] += a[e]; s[4 + e] += b[e]; }
    }
    bf16x8* o = (bf16x8*)(dx + i * 8);
    bf16x8 r;
    if (accum) {
      const bf16x8 old = *o;
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = (bf16)(s[e] + (float)old[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = (bf16)s[e];
    }
    *o = r;
  }
}

// ---- pre-packed DGRAD weights.  Every GEMM / halo DGRAD route reads the weights transposed
// ([ci][tap][co_p], taps flipped for the halo conv, split per parity phase at stride 2).  The
// optimizer re-packs every conv weight it owns right after its update, all of them in one
// launch (rtsds_conv2d_dgrad_pack_many), and the backward passes the packed copy with
// RTSDS_WEIGHT_PACKED instead of repacking per call (one tiny launch per conv and backward).
struct PackSeg {
  const void* w;
  void* wt;  // segment base (phase offset applied)
  int co_n, co_p, kh, kw, ci_n, tkh, tkw, r0h, r0w, rstep, blk0;
};
static const int kPackSegs = 16;
struct PackBatch {
  PackSeg s[kPackSegs];
  int nseg;
};
// One workgroup per (tap, 64 Cout x 64 Cin tile): rows of Cin read coalesced, transposed
// through LDS, rows of Cout written coalesced ([ci][tap][co_p], zero for co >= co_n).
static int pack_tiles(const PackSeg& q) { return q.tkh * q.tkw * rt_cdiv(q.co_p, 64) * rt_cdiv(q.ci_n, 64); }
template <typename T>
__global__ void __launch_bounds__(256) dgrad_pack_kernel(const PackBatch b) {
  __shared__ float tile[64][65];
  int si = 0;
  for (int i = 1; i < b.nseg; ++i)
    if (b.s[i].blk0 <= (int)blockIdx.x) si = i;
  const PackSeg& g = b.s[si];
  const int nco = (g.co_p + 63) / 64, nci = (g.ci_n + 63) / 64, taps = g.tkh * g.tkw;
  int t = (int)blockIdx.x - g.blk0;
  const int ct = t % nci;
  t /= nci;
  const int ot = t % nco, tap = t / nco;
  const int r = g.r0h + (tap / g.tkw) * g.rstep, sc = g.r0w + (tap % g.tkw) * g.rstep;
  const T* __restrict__ w = (const T*)g.w;
  T* __restrict__ wt = (T*)g.wt;
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  // clamped, unconditional loads, all 16 in flight (a guarded load per element serialised them:
  // one memory round trip each), then the zero fill of the padding selected
  T v[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int co = min(ot * 64 + ly + 4 * k, g.co_n - 1), ci = min(ct * 64 + lx, g.ci_n - 1);
    v[k] = w[((co * g.kh + r) * g.kw + sc) * g.ci_n + ci];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int co = ot * 64 + ly + 4 * k, ci = ct * 64 + lx;
    tile[ly + 4 * k][lx] = (co < g.co_n && ci < g.ci_n) ? to_f(v[k]) : 0.f;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int ci = ct * 64 + ly + 4 * k, co = ot * 64 + lx;
    if (ci < g.ci_n && co < g.co_p) wt[((long)ci * taps + tap) * g.co_p + co] = from_f<T>(tile[lx][ly + 4 * k]);
  }
}

// ---- host side ---------------------------------------------------------------------------
// The DGRAD route of a descriptor and its workspace, one plan for the query, the weight pre-pack
// and the launch: [repacked (and Cout-padded) weights][Cout-padded dY][split-K slabs].  The direct
// routes need no slabs, the pooled and narrow-1x1 routes no workspace; RTSDS_WEIGHT_PACKED leaves
// the weights region unused, not smaller.
enum DgradRoute {
  DG_POOLED,  // pooled vectors (conv_pooled.hip)
  DG_PW,      // narrow-output 1x1: direct FMA over dY rows (pw.hip)
  DG_TAP,     // 3x3 64 -> 64 stride 1: the register-resident-weight direct conv over dY (tapconv.hip)
  DG_HALO,    // narrow-output 3x3: the halo direct conv over dY (hconv.hip)
  DG_PHASES,  // stride 2: the parity phases, each a dense GEMM over only the taps that reach it
  DG_GEMM     // the implicit GEMM (with split-K slabs when dgrad_split() asks)
};
struct DgradPlan {
  DgradRoute route;
  int kp;  // Cout as the route reads it (padded to the vector width)
  size_t wt_bytes, dyp_bytes;
  DgradSplit split;
  size_t total() const { return wt_bytes + dyp_bytes + split.slab_bytes; }
  void* wt(void* ws) const { return ws; }
  void* dyp(void* ws) const { return (char*)ws + wt_bytes; }
  float* slab(void* ws) const { return (float*)((char*)ws + wt_bytes + dyp_bytes); }
};
static DgradPlan dgrad_plan(const rtsds_conv_desc* d) {
  DgradPlan pl = {DG_GEMM, pad_c(d->k, d->dtype), 0, 0, {1, 1 << 30, 0}};
  if (pooled_1x1(d) || pw_ok(d)) {
    pl.route = pooled_1x1(d) ? DG_POOLED : DG_PW;
    return pl;
  }
  const size_t es = esize(d->dtype);
  pl.wt_bytes = al256((size_t)pl.kp * d->kh * d->kw * d->c * es);
  if (pl.kp != d->k) pl.dyp_bytes = al256((size_t)d->n * d->ho * d->wo * pl.kp * es);
  if (tapconv_ok(d)) pl.route = DG_TAP;
  else if (pl.kp % 32 == 0 && hconv_dgrad_ok(d)) pl.route = DG_HALO;
  else {
    pl.split = dgrad_split(d, pl.kp);
    if (d->sh == 2 && d->sw == 2) pl.route = DG_PHASES;
  }
  return pl;
}
extern "C" size_t rtsds_conv2d_dgrad_workspace(const rtsds_conv_desc* d) { return dgrad_plan(d).total(); }

// Taps of one dgrad stride phase along an axis: input index i = t*2 + off receives from
// kernel taps r with (i + pad - r*dil) even.
static void phase_taps(int a, int pad, int dil, int ksz, int size, int& off, int& cnt_pix, int& r0, int& rstep, int& tk) {
  off = ((a - pad) % 2 + 2) % 2;
  cnt_pix = size > off ? (size - off + 1) / 2 : 0;
  if (dil % 2) { r0 = a; rstep = 2; tk = ksz > a ? (ksz - a + 1) / 2 : 0; }
  else { r0 = 0; rstep = 1; tk = a == 0 ? ksz : 0; }
}
// The stride-2 parity phases of d in launch order (returns how many, <= 4): the phase's taps
// r = r0 + rr*rstep (rr < tk), its hp x wp pixels ih = th*2 + offh, and the element offset boff of
// its repacked weights [ci][tap][kp].  A phase without pixels is skipped and takes no weights; one
// without taps stays (its pixels are zero-filled by the launch) with a zero-sized slot.
struct DgradPhase {
  int tkh, tkw, r0h, r0w, rstep, hp, wp, offh, offw;
  long boff;
};
static int dgrad_phases(const rtsds_conv_desc* d, int kp, DgradPhase* ph) {
  int n = 0;
  long boff = 0;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b) {
      DgradPhase q;
      int rsw;
      phase_taps(a, d->ph, d->dh, d->kh, d->h, q.offh, q.hp, q.r0h, q.rstep, q.tkh);
      phase_taps(b, d->pw, d->dw, d->kw, d->w, q.offw, q.wp, q.r0w, rsw, q.tkw);
      if (q.hp == 0 || q.wp == 0) continue;
      q.boff = boff;
      boff += (long)q.tkh * q.tkw * kp * d->c;
      ph[n++] = q;
    }
  return n;
}

// One segment of d's weight repack; wt holds the element offset until the caller adds the base.
static PackSeg pack_seg(const rtsds_conv_desc* d, int kp, int tkh, int tkw, int r0h, int r0w, int rstep, long boff) {
  PackSeg q = {};
  q.co_n = d->k; q.co_p = kp; q.kh = d->kh; q.kw = d->kw; q.ci_n = d->c;
  q.tkh = tkh; q.tkw = tkw; q.r0h = r0h; q.r0w = r0w; q.rstep = rstep;
  q.wt = (void*)(intptr_t)boff;
  return q;
}
// The routes without phases repack every tap at once; flipped for the direct convs, which run
// the forward kernel over dY.
static PackSeg pack_whole(const rtsds_conv_desc* d, const DgradPlan& pl) {
  if (pl.route == DG_GEMM) return pack_seg(d, pl.kp, d->kh, d->kw, 0, 0, 1, 0);
  return pack_seg(d, pl.kp, d->kh, d->kw, d->kh - 1, d->kw - 1, -1, 0);
}
// Segments of d's DGRAD weight repack (the layout dgrad_impl reads); 0 = no repack on its route.
static int dgrad_pack_plan(const rtsds_conv_desc* d, const DgradPlan& pl, PackSeg* seg) {
  switch (pl.route) {
    case DG_POOLED:
    case DG_PW: return 0;
    case DG_PHASES: {
      DgradPhase ph[4];
      const int nph = dgrad_phases(d, pl.kp, ph);
      int n = 0;
      for (int i = 0; i < nph; ++i)
        if (ph[i].tkh * ph[i].tkw > 0)
          seg[n++] = pack_seg(d, pl.kp, ph[i].tkh, ph[i].tkw, ph[i].r0h, ph[i].r0w, ph[i].rstep, ph[i].boff);
      return n;
    }
    case DG_GEMM:
      if (d->sh != 1 || d->sw != 1) return 0;  // (mixed strides: repacked per call only)
      break;
    case DG_TAP:
    case DG_HALO: break;
  }
  seg[0] = pack_whole(d, pl);
  return 1;
}
extern "C" size_t rtsds_conv2d_dgrad_pack_bytes(const rtsds_conv_desc* d) {
  if (check_desc(d)) return 0;
  PackSeg seg[4];
  const DgradPlan pl = dgrad_plan(d);
  return dgrad_pack_plan(d, pl, seg) ? pl.wt_bytes : 0;
}
extern "C" int rtsds_conv2d_dgrad_pack_many(int count, const rtsds_conv_desc* descs, const void* const* w, void* const* wt,
                                            void* stream) {
  hipStream_t st = (hipStream_t)stream;
  PackBatch b = {};
  int blocks = 0, dtype = -1;
  auto flush = [&]() -> int {
    if (b.nseg == 0) return RTSDS_OK;
    DISPATCH_T(dtype, hipLaunchKernelGGL(dgrad_pack_kernel<T>, dim3(blocks), dim3(256), 0, st, b));
    b.nseg = 0;
    blocks = 0;
    return RTSDS_OK;
  };
  for (int i = 0; i < count; ++i) {
    const rtsds_conv_desc* d = descs + i;
    if (check_desc(d) || !w[i] || !wt[i]) return RTSDS_ERR_SHAPE;
    PackSeg seg[4];
    const int n = dgrad_pack_plan(d, dgrad_plan(d), seg);
    if (n == 0) return RTSDS_ERR_UNSUPPORTED;
    if (d->dtype != dtype || b.nseg + n > kPackSegs)
      if (int e = flush()) return e;
    dtype = d->dtype;
    for (int j = 0; j < n; ++j) {
      PackSeg q = seg[j];
      q.w = w[i];
      q.wt = (char*)wt[i] + (intptr_t)q.wt * esize(d->dtype);
      q.blk0 = blocks;
      blocks += pack_tiles(q);
      b.s[b.nseg++] = q;
    }
  }
  if (int e = flush()) return e;
  RET_LAUNCH();
}
// The per-call repack of one segment (no RTSDS_WEIGHT_PACKED).
static int repack_launch(int dtype, const void* w, void* wt, const PackSeg& q, hipStream_t st) {
  const long wn = (long)q.co_p * q.tkh * q.tkw * q.ci_n;
  if (wn <= 0) return RTSDS_OK;
  const int blocks = (int)std::min<long>(4096, (wn + 255) / 256);
  DISPATCH_T(dtype, hipLaunchKernelGGL(repack_wt_kernel<T>, dim3(blocks), dim3(256), 0, st, (const T*)w, (T*)wt, q.co_n, q.co_p,
                                       q.kh, q.kw, q.ci_n, q.tkh, q.tkw, q.r0h, q.r0w, q.rstep));
  return RTSDS_OK;
}

// mask: see ConvArgs::mask.  Paths whose epilogue does not apply it (pooled, narrow 1x1, halo,
// split-K) report false and the caller masks dx in place afterwards.
struct BnbArgs {  // see ConvArgs::bnb_part
  float* part;
  const void* x;
  const float *gamma, *beta, *mean, *invstd;
  int act;
};
static int dgrad_impl(const rtsds_conv_desc* d0, const void* dy, const void* w, void* dx, int accumulate, const void* mask,
                      int mask_act, bool& masked, void* ws, size_t ws_bytes, void* stream, const BnbArgs* bnb = nullptr,
                      bool packed = false) {
  masked = false;
  int e = check_desc(d0);
  if (e) return e;
  if (d0->sh > 2 || d0->sw > 2) return RTSDS_ERR_UNSUPPORTED;
  const DgradPlan pl = dgrad_plan(d0);
  if (ws_bytes < pl.total()) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (pl.route == DG_POOLED) return pooled_dgrad(d0, dy, w, dx, accumulate ? 1 : 0, st);
  if (pl.route == DG_PW) {
    pw_dgrad(d0, dy, w, dx, accumulate ? 1 : 0, st);
    RET_LAUNCH();
  }
  rtsds_conv_desc d = *d0;
  const int kp = pl.kp, k_real = d.k;
  // packed: w already is the transposed copy (rtsds_conv2d_dgrad_pack_many); else repack it here
  void* wt = packed ? const_cast<void*>(w) : pl.wt(ws);
  if (pl.dyp_bytes) {
    if ((e = pad_any(d.dtype, dy, pl.dyp(ws), (long)d.n * d.ho * d.wo, d.k, kp, st))) return e;
    dy = pl.dyp(ws);
  }
  d.k = kp;
  if (pl.route != DG_PHASES && !packed && (e = repack_launch(d.dtype, w, wt, pack_whole(d0, pl), st))) return e;
  if (pl.route == DG_TAP) {  // mask / accumulate / BatchNorm backward statistics in its epilogue
    tapconv_dgrad(d0, dy, wt, dx, accumulate, mask, mask_act, bnb ? bnb->part : nullptr, bnb ? bnb->x : nullptr,
                  bnb ? bnb->gamma : nullptr, bnb ? bnb->beta : nullptr, bnb ? bnb->mean : nullptr,
                  bnb ? bnb->invstd : nullptr, bnb ? bnb->act : 0, st);
    masked = mask != nullptr;
    RET_LAUNCH();
  }
  if (pl.route == DG_HALO) {
    hconv_dgrad(d0, dy, kp, wt, dx, accumulate, st);
    RET_LAUNCH();
  }
  ConvArgs p = make_args(&d);
  p.a = dy; p.b = wt; p.bias = nullptr; p.out = dx; p.act = 0;
  p.accum = accumulate ? 1 : 0;
  p.mask = mask;
  p.mask_act = mask_act;
  p.N = d.c;
  if (pl.route == DG_PHASES) {
    // the phases' weights repacked by one launch, the phases computed by one launch (blockIdx.z = phase)
    masked = mask != nullptr;
    p.psh = 2;
    DgradPhase ph[4];
    const int nph = dgrad_phases(d0, kp, ph);
    if (nph == 0) return RTSDS_OK;
    RepackPhases rp = {};
    int max_m = 0, max_w = 0;
    for (int i = 0; i < nph; ++i) {
      const DgradPhase& s = ph[i];
      ConvArgs::Phase& q = p.phs[i];
      q.hp = s.hp; q.wp = s.wp; q.offh = s.offh; q.offw = s.offw; q.r0h = s.r0h; q.r0w = s.r0w;
      q.tkw = s.tkw > 0 ? s.tkw : 1;
      q.f_tkw = fastdiv_make(q.tkw);
      q.f_hw = fastdiv_make(s.hp * s.wp);
      q.f_w = fastdiv_make(s.wp);
      q.M = d.n * s.hp * s.wp;
      q.K = s.tkh * s.tkw * kp;
      q.boff = s.boff;
      rp.tkh[i] = s.tkh; rp.tkw[i] = s.tkw; rp.r0h[i] = s.r0h; rp.r0w[i] = s.r0w; rp.boff[i] = s.boff;
      max_m = std::max(max_m, q.M);
      max_w = std::max(max_w, q.K * d.c);
    }
    const int rstep = ph[nph - 1].rstep;  // (the same in every phase: it follows the dilation's parity)
    if (max_w > 0 && !packed) {
      const dim3 g(std::min(4096, (max_w + 255) / 256), nph);
      DISPATCH_T(d.dtype, hipLaunchKernelGGL(repack_phases_kernel<T>, g, dim3(256), 0, st, (const T*)w, (T*)wt, k_real, kp, d.kh,
                                             d.kw, d.c, rstep, rp));
    }
    // shared fields: the first phase's (tile choice and alignment class depend only on M, N, kp)
    p.nph = nph;
    p.hp = p.phs[0].hp; p.wp = p.phs[0].wp; p.offh = p.phs[0].offh; p.offw = p.phs[0].offw;
    p.r0h = p.phs[0].r0h; p.r0w = p.phs[0].r0w; p.rstep = rstep; p.tkw = p.phs[0].tkw;
    p.f_tkw = p.phs[0].f_tkw; p.f_hw = p.phs[0].f_hw; p.f_w = p.phs[0].f_w;
    p.M = max_m;
    p.K = p.phs[0].K;
    DISPATCH_T(d.dtype, dispatch_align<T, MODE_DGRAD>(p, kp, st));
    RET_LAUNCH();
  }
  if (bnb) {  // (rtsds_conv2d_dgrad_bnstats_tiles checked this route)
    p.bnb_part = bnb->part; p.bnb_x = bnb->x; p.bnb_gamma = bnb->gamma; p.bnb_beta = bnb->beta;
    p.bnb_mean = bnb->mean; p.bnb_invstd = bnb->invstd; p.bnb_act = bnb->act;
  }
  p.M = d.n * d.h * d.w;
  p.K = d.kh * d.kw * kp;
  if (pl.split.splits > 1) {
    p.slab = pl.slab(ws);
    p.split_stride = (long)p.M * p.N;
    p.tiles_per_split = pl.split.tps;
    p.accum = 0;
    p.mask = nullptr;  // the split reduce writes dx: masked afterwards by the caller
    launch_al<bf16, MODE_DGRAD, 128, 128, 64, 2, 2>(p, kp, st, pl.split.splits);
    const long nv8 = (long)p.M * p.N / 8;
    hipLaunchKernelGGL(dgrad_split_reduce_kernel, dim3((int)std::min<long>(8192, (nv8 + 255) / 256)), dim3(256), 0, st,
                       (const float*)p.slab, (bf16*)dx, nv8, p.split_stride, pl.split.splits, accumulate ? 1 : 0);
    RET_LAUNCH();
  }
  masked = mask != nullptr;
  DISPATCH_T(d.dtype, dispatch_align<T, MODE_DGRAD>(p, kp, st));
  RET_LAUNCH();
}

extern "C" int rtsds_conv2d_dgrad(const rtsds_conv_desc* d0, const void* dy, const void* w, void* dx,
                                  int accumulate, void* ws, size_t ws_bytes, void* stream) {
  bool masked = false;
  const bool packed = (accumulate & RTSDS_WEIGHT_PACKED) != 0;
  return dgrad_impl(d0, dy, w, dx, accumulate & ~RTSDS_WEIGHT_PACKED, nullptr, 0, masked, ws, ws_bytes, stream, nullptr,
                    packed);
}
// M tiles of the data-gradient GEMM when its epilogue can emit the BatchNorm backward
// statistics (bf16, stride 1, plain GEMM path: not the pooled / narrow-1x1 / halo / split-K
// routes, vector epilogue), else 0.  (The stride-2 parity-phase launch could carry them too:
// measured for the spatial path's BatchNorms, the epilogue cost what the statistics pass saved.)
extern "C" int rtsds_conv2d_dgrad_bnstats_tiles(const rtsds_conv_desc* d) {
  if (check_desc(d) || d->dtype != RTSDS_BF16 || d->sh != 1 || d->sw != 1 || d->c % 8 != 0) return 0;
  const DgradPlan pl = dgrad_plan(d);
  if (pl.route == DG_TAP) return tapconv_rows(d, 1);
  if (pl.route != DG_GEMM || pl.split.splits > 1) return 0;
  int bm, bn;
  const long M = (long)d->n * d->h * d->w;
  pick_tile(M, d->c, true, bm, bn, false, (long)d->kh * d->kw * pl.kp, true);  // dispatch_align's choice
  if (256 % (bn / 8) != 0) return 0;
  return (int)((M + bm - 1) / bm);
}
extern "C" int rtsds_conv2d_dgrad_bnstats(const rtsds_conv_desc* d0, const void* dy, const void* w, void* dx, const void* bn_x,
                                          const float* gamma, const float* beta, const float* save_mean,
                                          const float* save_invstd, int act, float* part, void* ws, size_t ws_bytes,
                                          void* stream) {
  const bool packed = (act & RTSDS_WEIGHT_PACKED) != 0;
  act &= ~RTSDS_WEIGHT_PACKED;
  if (rtsds_conv2d_dgrad_bnstats_tiles(d0) == 0) return RTSDS_ERR_UNSUPPORTED;
  if (!bn_x || !save_mean || !save_invstd || !part || (act != RTSDS_ACT_NONE && act != RTSDS_ACT_RELU && act != RTSDS_ACT_LEAKY))
    return RTSDS_ERR_UNSUPPORTED;
  const BnbArgs b = {part, bn_x, gamma, beta, save_mean, save_invstd, act};
  bool masked = false;
  return dgrad_impl(d0, dy, w, dx, 0, nullptr, 0, masked, ws, ws_bytes, stream, &b, packed);
}
extern "C" int rtsds_conv2d_dgrad_act(const rtsds_conv_desc* d0, const void* dy, const void* w, void* dx, const void* x_act,
                                      int act, void* ws, size_t ws_bytes, void* stream) {
  const bool packed = (act & RTSDS_WEIGHT_PACKED) != 0;
  act &= ~RTSDS_WEIGHT_PACKED;
  if (!x_act || (act != RTSDS_ACT_RELU && act != RTSDS_ACT_LEAKY)) return RTSDS_ERR_UNSUPPORTED;
  bool masked = false;
  const int e = dgrad_impl(d0, dy, w, dx, 0, x_act, act, masked, ws, ws_bytes, stream, nullptr, packed);
  if (e || masked) return e;
  return rtsds_act_bwd(dx, x_act, dx, (long)d0->n * d0->h * d0->w * d0->c, act, 1.f, d0->dtype, stream);
}
