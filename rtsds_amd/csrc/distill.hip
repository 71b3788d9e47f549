// Knowledge distillation on the low-resolution main heads (no reference counterpart; protocol in
// include/rtsds_hip.h and functional.distill_kl): the teacher's logits are resampled bilinearly
// onto the student's grid, both rows are softened by 1/T, and the pixel's KL(p || q), the residual
// q - p and the argmax agreement are formed in one pass.  Neither the resampled logits nor the
// probabilities are written to memory.
#include "class_row.h"
#include "row_stage.h"

static const int kKdPix = 128;             // pixels of a tile = threads of a workgroup: one run inside one student row
static const int kKdCMax = 32;
static const size_t kKdLdsCap = 64 * 1024;
static const int kKdRed = 16;              // bytes in front of the tiles: one loss sum per wave

// common.h bil_mix with a tap of weight zero left out: for finite taps the same bits (0 * p + 1 * q
// is q), and a teacher's -inf (a masked class) under a zero weight -- every second tap of equal
// sizes -- does not turn the blend into NaN.
RT_DEV float kd_mix(float p00, float p01, float p10, float p11, float lh0, float lh1, float lw0, float lw1) {
  const float t0 = lw1 == 0.f ? p00 : fmaf(lw1, p01, lw0 * p00);
  const float t1 = lw1 == 0.f ? p10 : fmaf(lw1, p11, lw0 * p10);
  return lh1 == 0.f ? t0 : fmaf(lh1, t1, lh0 * t0);
}

struct KdArgs {
  const void* s;
  const void* t;
  int hs, ws, ht, wt, c;
  float sh, sw, inv_temp;
  int tiles_x;  // tiles per student row
  int cap;      // teacher columns per staged source row that the LDS holds (0: nothing is staged)
  int want_grad;
  float* part;  // [blocks] loss partials
  float* resid; // [n][hs][ws][c] q - p
  unsigned long long* agree;
};

// One workgroup per tile of <= kKdPix consecutive pixels of one student row; block b = (image row, tile).
// Dynamic LDS (all of the kernel's LDS, so its base stays 16-B aligned): the waves' loss sums | student
// tile | residual tile | the teacher's two source rows over the tile's span.
template <typename Ts, typename Tt, int CC>
__global__ void __launch_bounds__(kKdPix) kd_fwd_kernel(KdArgs a) {
  constexpr int MAXC = CC ? CC : kKdCMax;
  const int c = CC ? CC : a.c;
  const int tid = threadIdx.x;
  const int row = blockIdx.x / a.tiles_x, tile = blockIdx.x - row * a.tiles_x;  // row = image * hs + y
  const int img = row / a.hs, y = row - img * a.hs;
  const int x0 = tile * kKdPix, np = min(kKdPix, a.ws - x0);

  float* red = stage_buf<float>();
  char* lds = (char*)red + kKdRed;
  Ts* sbuf = (Ts*)lds;
  float* rbuf = (float*)(lds + rs_lds_row((size_t)kKdPix * c, sizeof(Ts)));
  Tt* tbuf0 = (Tt*)((char*)rbuf + rs_lds_row((size_t)kKdPix * c, sizeof(float)));
  Tt* tbuf1 = (Tt*)((char*)tbuf0 + rs_lds_row((size_t)a.cap * c, sizeof(Tt)));

  int ih0, ih1, c0, c1, unused;
  float lh0, lh1, lu0, lu1;
  bil_src(y, a.sh, a.ht, ih0, ih1, lh0, lh1);
  bil_src(x0, a.sw, a.wt, c0, unused, lu0, lu1);           // the taps are non-decreasing in x, so the
  bil_src(x0 + np - 1, a.sw, a.wt, unused, c1, lu0, lu1);  // tile's source columns are c0 .. c1
  const int nsp = c1 - c0 + 1;
  const bool staged = nsp <= a.cap;  // the same for the whole workgroup

  const Ts* sg = (const Ts*)a.s + ((long)row * a.ws + x0) * c;
  const Tt* tg0 = (const Tt*)a.t + (((long)img * a.ht + ih0) * a.wt) * c;  // the source rows, column 0
  const Tt* tg1 = (const Tt*)a.t + (((long)img * a.ht + ih1) * a.wt) * c;
  rs_in(sg, sbuf, np * c);
  if (staged) {
    rs_in(tg0 + (long)c0 * c, tbuf0, nsp * c);
    rs_in(tg1 + (long)c0 * c, tbuf1, nsp * c);
  }
  float* rg = a.resid + ((long)row * a.ws + x0) * c;
  const int rlead = rs_lead(rg);
  __syncthreads();

  float kl = 0.f;
  bool same = false;
  if (tid < np) {
    int iw0, iw1;
    float lw0, lw1;
    bil_src(x0 + tid, a.sw, a.wt, iw0, iw1, lw0, lw1);
    const Ts* sp = sbuf + rs_lead(sg) + tid * c;
    float va[MAXC], vb[MAXC], ea[MAXC], eb[MAXC];
    // r0 / r1: the two source rows at column `first`, in LDS or in memory
    auto rows = [&](const Tt* r0, const Tt* r1, int first) {
      const Tt *p00 = r0 + (long)(iw0 - first) * c, *p01 = r0 + (long)(iw1 - first) * c;
      const Tt *p10 = r1 + (long)(iw0 - first) * c, *p11 = r1 + (long)(iw1 - first) * c;
#pragma unroll
      for (int k = 0; k < MAXC; ++k)
        if (k < c) vb[k] = kd_mix(to_f(p00[k]), to_f(p01[k]), to_f(p10[k]), to_f(p11[k]), lh0, lh1, lw0, lw1);
    };
    if (staged) rows(tbuf0 + rs_lead(tg0 + (long)c0 * c), tbuf1 + rs_lead(tg1 + (long)c0 * c), c0);
    else rows(tg0, tg1, 0);
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < c) va[k] = to_f(sp[k]);
    float best;
    same = first_max<MAXC>([&](int k) { return va[k]; }, c, best) == first_max<MAXC>([&](int k) { return vb[k]; }, c, best);
    float za, lza, zb, lzb;
    rs_soften<MAXC>(va, ea, c, a.inv_temp, za, lza);
    rs_soften<MAXC>(vb, eb, c, a.inv_temp, zb, lzb);
    float* rp = rbuf + rlead + tid * c;
#pragma unroll
    for (int k = 0; k < MAXC; ++k)
      if (k < c) {
        const float q = ea[k] / za, p = eb[k] / zb;
        const float d = __fsub_rn(__fsub_rn(vb[k], lzb), __fsub_rn(va[k], lza));
        kl = __fadd_rn(kl, p == 0.f ? 0.f : __fmul_rn(p, d));  // torch's xlogy rule
        rp[k] = __fsub_rn(q, p);
      }
  }

  const float wsum = wave_sum(kl);
  const unsigned long long votes = __ballot(same);
  if ((tid & 63) == 0) {
    red[tid >> 6] = wsum;
    if (a.agree && votes) atomicAdd(a.agree, (unsigned long long)__popcll(votes));
  }
  __syncthreads();  // also: the residual tile is complete
  if (tid == 0) a.part[blockIdx.x] = red[0] + red[1];
  if (a.want_grad) rs_out(rg, rbuf, np * c);
}

// ------------------------------------------------------------------ host
struct KdPlan {
  int blocks, tiles_x, cap;
  size_t lds, part_bytes, resid_bytes;
};
static size_t kd_elem(int dtype) { return dtype == RTSDS_BF16 ? 2 : 4; }
static bool kd_shape_ok(int n, int hs, int ws, int c, int ht, int wt) {
  if (n < 1 || hs < 1 || ws < 1 || ht < 1 || wt < 1 || c < 2 || c > kKdCMax) return false;
  const long lim = 1L << 31;
  return (long)n * hs * ws * c < lim && (long)n * ht * wt * c < lim && (long)n * hs * rt_cdiv(ws, kKdPix) < lim;
}
// The geometry of a launch.  The teacher's source rows are staged when two rows of the widest span a
// tile can have (cap columns: bil_src moves at most scale_w per pixel, plus the second tap and slack
// for the fp32 rounding) fit the LDS beside the student and residual tiles; else cap = 0 and every
// tile reads its taps from memory.  The kernel compares each tile's span with cap itself.
static KdPlan kd_plan(int n, int hs, int ws, int c, int wt, float scale_w, size_t s_elem, size_t t_elem) {
  KdPlan p;
  p.tiles_x = rt_cdiv(ws, kKdPix);
  p.blocks = n * hs * p.tiles_x;
  p.part_bytes = ((size_t)p.blocks * sizeof(float) + 15) & ~(size_t)15;
  p.resid_bytes = (size_t)n * hs * ws * c * sizeof(float);
  const size_t own = kKdRed + rs_lds_row((size_t)kKdPix * c, s_elem) + rs_lds_row((size_t)kKdPix * c, sizeof(float));
  const double span = std::ceil((double)scale_w * (std::min(ws, kKdPix) - 1)) + 4.0;
  p.cap = (int)std::min<double>(wt, span);
  p.lds = own + 2 * rs_lds_row((size_t)p.cap * c, t_elem);
  if (p.lds > kKdLdsCap) {
    p.cap = 0;
    p.lds = own + 2 * rs_lds_row(0, t_elem);
  }
  return p;
}

extern "C" size_t rtsds_distill_workspace(int n, int hs, int ws, int c, int ht, int wt) {
  if (!kd_shape_ok(n, hs, ws, c, ht, wt)) return 0;
  const KdPlan p = kd_plan(n, hs, ws, c, wt, 1.f, 4, 4);
  return p.part_bytes + p.resid_bytes;
}

static bool kd_dtype_ok(int d) { return d == RTSDS_F32 || d == RTSDS_BF16; }

extern "C" int rtsds_distill_fwd(const void* s, int s_dtype, const void* t, int t_dtype, int n, int hs, int ws, int c, int ht, int wt,
                                 float scale_h, float scale_w, float inv_temp, int want_grad, unsigned long long* agree, void* wsp,
                                 size_t ws_bytes, void* stream) {
  if (!s || !t || !kd_shape_ok(n, hs, ws, c, ht, wt)) return RTSDS_ERR_SHAPE;
  if (!(scale_h > 0.f) || !(scale_w > 0.f) || !std::isfinite(scale_h) || !std::isfinite(scale_w) || !(inv_temp > 0.f) ||
      !std::isfinite(inv_temp))
    return RTSDS_ERR_SHAPE;
  if (!kd_dtype_ok(s_dtype) || !kd_dtype_ok(t_dtype)) return RTSDS_ERR_UNSUPPORTED;
  if (((uintptr_t)s % kd_elem(s_dtype)) || ((uintptr_t)t % kd_elem(t_dtype)) || ((uintptr_t)wsp & 15) || ((uintptr_t)agree & 7))
    return RTSDS_ERR_UNSUPPORTED;
  if (!wsp || ws_bytes < rtsds_distill_workspace(n, hs, ws, c, ht, wt)) return RTSDS_ERR_WORKSPACE;
  const KdPlan p = kd_plan(n, hs, ws, c, wt, scale_w, kd_elem(s_dtype), kd_elem(t_dtype));
  KdArgs a;
  a.s = s; a.t = t;
  a.hs = hs; a.ws = ws; a.ht = ht; a.wt = wt; a.c = c;
  a.sh = scale_h; a.sw = scale_w; a.inv_temp = inv_temp;
  a.tiles_x = p.tiles_x;
  a.cap = p.cap;
  a.want_grad = want_grad != 0;
  a.part = (float*)wsp;
  a.resid = (float*)((char*)wsp + p.part_bytes);
  a.agree = agree;
  hipStream_t st = (hipStream_t)stream;
#define KD_LAUNCH(TS, TT)                                                                                       \
  do {                                                                                                          \
    if (c == 19) hipLaunchKernelGGL((kd_fwd_kernel<TS, TT, 19>), dim3(p.blocks), dim3(kKdPix), p.lds, st, a);   \
    else hipLaunchKernelGGL((kd_fwd_kernel<TS, TT, 0>), dim3(p.blocks), dim3(kKdPix), p.lds, st, a);            \
  } while (0)
  if (s_dtype == RTSDS_BF16 && t_dtype == RTSDS_BF16) KD_LAUNCH(bf16, bf16);
  else if (s_dtype == RTSDS_BF16) KD_LAUNCH(bf16, float);
  else if (t_dtype == RTSDS_BF16) KD_LAUNCH(float, bf16);
  else KD_LAUNCH(float, float);
#undef KD_LAUNCH
  RET_LAUNCH();
}

extern "C" int rtsds_distill_finish(const void* wsp, size_t ws_bytes, int n, int hs, int ws, double coef, float* loss, void* stream) {
  if (!loss || n < 1 || hs < 1 || ws < 1 || (long)n * hs * rt_cdiv(ws, kKdPix) >= (1L << 31) || !std::isfinite(coef))
    return RTSDS_ERR_SHAPE;
  if ((uintptr_t)wsp & 15) return RTSDS_ERR_UNSUPPORTED;
  const int blocks = n * hs * rt_cdiv(ws, kKdPix);
  if (!wsp || ws_bytes < (size_t)blocks * sizeof(float)) return RTSDS_ERR_WORKSPACE;
  hipLaunchKernelGGL(rs_finish_kernel<1>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)wsp, blocks, coef, RsOuts<1>{{loss}});
  RET_LAUNCH();
}

extern "C" int rtsds_distill_bwd(const void* wsp, size_t ws_bytes, const float* grad_loss, double coef_g, void* dx, int dtype, int n,
                                 int hs, int ws, int c, void* stream) {
  if (!grad_loss || !dx || !kd_shape_ok(n, hs, ws, c, 1, 1) || !std::isfinite(coef_g)) return RTSDS_ERR_SHAPE;
  if (!kd_dtype_ok(dtype) || ((uintptr_t)dx % kd_elem(dtype)) || ((uintptr_t)wsp & 15) || ((uintptr_t)grad_loss & 3))
    return RTSDS_ERR_UNSUPPORTED;
  if (!wsp || ws_bytes < rtsds_distill_workspace(n, hs, ws, c, 1, 1)) return RTSDS_ERR_WORKSPACE;
  const KdPlan p = kd_plan(n, hs, ws, c, 1, 1.f, 4, 4);
  const float* resid = (const float*)((const char*)wsp + p.part_bytes);
  const long total = (long)n * hs * ws * c;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(rs_bwd_kernel<T>, dim3(ew_blocks(total / VecT<T>::N + 2)), dim3(256), 0, st, resid, grad_loss,
                                       coef_g, (T*)dx, total));
  RET_LAUNCH();
}
