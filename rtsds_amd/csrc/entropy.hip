// Target entropy minimisation on the low-resolution main head (no reference counterpart; protocol
// in include/rtsds_hip.h and functional.entropy_loss): per pixel the softmax of the class row, its
// normalised Shannon entropy h and sum of squares S, one of three penalties of them -- h (ADVENT
// MinEnt), (h^2 + 1e-8)^eta (FDA's robust entropy), -S / 2 (Maximum Squares) -- and the penalty's
// closed-form gradient with respect to the logits, in one pass.  The probabilities never reach memory.
#include "row_stage.h"

static const int kEmPix = 128;  // pixels of a tile: consecutive pixels of the flattened [n h w] list
static const int kEmLanes = 2;  // adjacent lanes that share a pixel (tools/probe/entropy_lanes.hip times 1, 2 and 4)
static const int kEmCMax = 32;
static const int kEmRed = 64;   // bytes in front of the tiles: per wave (up to 8) one penalty sum and one entropy sum

struct EmArgs {
  const void* x;
  long pixels;
  int c, penalty, want_grad;
  float eta, inv_lnc;
  float* part;  // [blocks][2]: sum of the penalty, sum of h
  float* term;  // [pixels][c] d(penalty) / d(logit)
  float* hmap;  // [pixels] h, or NULL
};

// v + its partners' values over the L adjacent lanes of a pixel: xor steps 1, 2, .. -- a fixed
// order, and every lane of the group ends with the same bits.
template <int L>
RT_DEV float em_join(float v) {
#pragma unroll
  for (int o = 1; o < L; o <<= 1) v = __fadd_rn(v, __shfl_xor(v, o, 64));
  return v;
}

// One workgroup per tile of <= kEmPix consecutive pixels, L adjacent lanes per pixel: lane `sub`
// keeps classes sub, sub + L, .. in registers (a slot beyond c holds -inf, whose probability is 0),
// and the row's maximum, Z, sum p log p and S are joined across the L lanes.  L = 1 is a thread per
// pixel with sums in class order.  Dynamic LDS (all of the kernel's LDS, so its base stays 16-B
// aligned): the waves' sums | input tile | gradient-term tile.
template <typename T, int CC, int L>
__global__ void __launch_bounds__(kEmPix* L) em_fwd_kernel(EmArgs a) {
  constexpr int PER = ((CC ? CC : kEmCMax) + L - 1) / L;
  constexpr int NW = kEmPix * L / 64;
  const int c = CC ? CC : a.c;
  const int tid = threadIdx.x, pix = tid / L, sub = tid % L;
  const long p0 = (long)blockIdx.x * kEmPix;
  const int np = (int)min<long>(kEmPix, a.pixels - p0);

  float* red = stage_buf<float>();
  char* lds = (char*)red + kEmRed;
  T* xbuf = (T*)lds;
  float* tbuf = (float*)(lds + rs_lds_row((size_t)kEmPix * c, sizeof(T)));

  const T* xg = (const T*)a.x + p0 * c;
  rs_in(xg, xbuf, np * c);
  float* tg = a.term + p0 * c;
  const int tlead = rs_lead(tg);
  __syncthreads();

  float phi = 0.f, hn = 0.f;
  if (pix < np) {  // the L lanes of a pixel agree on this, so every shuffle below has its partners
    const T* xp = xbuf + rs_lead(xg) + pix * c;
    float v[PER], e[PER];
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const int k = sub + i * L;
      v[i] = k < c ? to_f(xp[k]) : -INFINITY;
      m = fmaxf(m, v[i]);
    }
#pragma unroll
    for (int o = 1; o < L; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    float z = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      v[i] = __fsub_rn(v[i], m);
      e[i] = expf(v[i]);
      z = __fadd_rn(z, e[i]);
    }
    z = em_join<L>(z);
    const float lz = logf(z);
    // e <- p, v <- log p; acc = sum p log p (xlogy rule), sq = sum p^2
    float acc = 0.f, sq = 0.f;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
      const float p = e[i] / z, lp = __fsub_rn(v[i], lz);
      e[i] = p;
      v[i] = lp;
      acc = __fadd_rn(acc, p == 0.f ? 0.f : __fmul_rn(p, lp));
      sq = __fadd_rn(sq, __fmul_rn(p, p));
    }
    acc = em_join<L>(acc);
    sq = em_join<L>(sq);
    const float ent = -acc;
    hn = fminf(__fmul_rn(ent, a.inv_lnc), 1.f);
    float* tp = tbuf + tlead + pix * c;
    if (a.penalty == RTSDS_ENTROPY_MAX_SQUARES) {
      phi = __fmul_rn(-0.5f, sq);
      if (a.want_grad) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          const int k = sub + i * L;
          if (k < c) tp[k] = e[i] == 0.f ? 0.f : -__fmul_rn(e[i], __fsub_rn(e[i], sq));
        }
      }
    } else {
      float f = 1.f;  // d(penalty) / dh
      phi = hn;
      if (a.penalty == RTSDS_ENTROPY_ROBUST) {
        const float u = __fadd_rn(__fmul_rn(hn, hn), 1e-8f);
        const bool two = a.eta == 2.f;
        phi = two ? __fmul_rn(u, u) : powf(u, a.eta);
        f = __fmul_rn(__fmul_rn(2.f * a.eta, hn), two ? u : powf(u, a.eta - 1.f));
      }
      if (a.want_grad) {
#pragma unroll
        for (int i = 0; i < PER; ++i) {
          const int k = sub + i * L;
          if (k < c) {
            const float b = e[i] == 0.f ? 0.f : -__fmul_rn(__fmul_rn(e[i], __fadd_rn(v[i], ent)), a.inv_lnc);
            tp[k] = __fmul_rn(f, b);
          }
        }
      }
    }
    if (sub) phi = hn = 0.f;  // one lane of the pixel speaks for it
    else if (a.hmap) a.hmap[p0 + pix] = hn;
  }

  const float wphi = wave_sum(phi), wh = wave_sum(hn);
  if ((tid & 63) == 0) {
    red[tid >> 6] = wphi;
    red[NW + (tid >> 6)] = wh;
  }
  __syncthreads();  // also: the gradient-term tile is complete
  if (tid == 0) {
    float s0 = red[0], s1 = red[NW];
#pragma unroll
    for (int i = 1; i < NW; ++i) {
      s0 += red[i];
      s1 += red[NW + i];
    }
    a.part[2 * (long)blockIdx.x] = s0;
    a.part[2 * (long)blockIdx.x + 1] = s1;
  }
  if (a.want_grad) rs_out(tg, tbuf, np * c);
}

// ------------------------------------------------------------------ host
struct EmPlan {
  int blocks;
  size_t part_bytes, term_bytes;
};
static size_t em_elem(int dtype) { return dtype == RTSDS_BF16 ? 2 : 4; }
static bool em_dtype_ok(int d) { return d == RTSDS_F32 || d == RTSDS_BF16; }
static bool em_shape_ok(int n, int h, int w, int c) {
  if (n < 1 || h < 1 || w < 1 || c < 2 || c > kEmCMax) return false;
  const long lim = 1L << 31;
  return (long)n * h < lim && (long)n * h * w < lim && (long)n * h * w * c < lim;
}
static EmPlan em_plan(int n, int h, int w, int c) {
  EmPlan p;
  const long pixels = (long)n * h * w;
  p.blocks = (int)((pixels + kEmPix - 1) / kEmPix);
  p.part_bytes = ((size_t)p.blocks * 2 * sizeof(float) + 15) & ~(size_t)15;
  p.term_bytes = (size_t)pixels * c * sizeof(float);
  return p;
}
static size_t em_lds(int c, size_t elem) {
  return kEmRed + rs_lds_row((size_t)kEmPix * c, elem) + rs_lds_row((size_t)kEmPix * c, sizeof(float));
}

extern "C" size_t rtsds_entropy_workspace(int n, int h, int w, int c) {
  if (!em_shape_ok(n, h, w, c)) return 0;
  const EmPlan p = em_plan(n, h, w, c);
  return p.part_bytes + p.term_bytes;
}

extern "C" int rtsds_entropy_fwd(const void* x, int dtype, int n, int h, int w, int c, int penalty, float eta, int want_grad,
                                 float* hmap, void* wsp, size_t ws_bytes, void* stream) {
  if (!x || !em_shape_ok(n, h, w, c)) return RTSDS_ERR_SHAPE;
  if (penalty != RTSDS_ENTROPY_ENTROPY && penalty != RTSDS_ENTROPY_ROBUST && penalty != RTSDS_ENTROPY_MAX_SQUARES)
    return RTSDS_ERR_SHAPE;
  if (!(eta > 0.f) || !std::isfinite(eta)) return RTSDS_ERR_SHAPE;
  if (!em_dtype_ok(dtype)) return RTSDS_ERR_UNSUPPORTED;
  if (((uintptr_t)x % em_elem(dtype)) || ((uintptr_t)wsp & 15) || ((uintptr_t)hmap & 3)) return RTSDS_ERR_UNSUPPORTED;
  if (!wsp || ws_bytes < rtsds_entropy_workspace(n, h, w, c)) return RTSDS_ERR_WORKSPACE;
  const EmPlan p = em_plan(n, h, w, c);
  EmArgs a;
  a.x = x;
  a.pixels = (long)n * h * w;
  a.c = c; a.penalty = penalty; a.want_grad = want_grad != 0;
  a.eta = eta;
  a.inv_lnc = (float)(1.0 / std::log((double)c));
  a.part = (float*)wsp;
  a.term = (float*)((char*)wsp + p.part_bytes);
  a.hmap = hmap;
  const size_t lds = em_lds(c, em_elem(dtype));
  const dim3 threads(kEmPix * kEmLanes);
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, {
    if (c == 19) hipLaunchKernelGGL((em_fwd_kernel<T, 19, kEmLanes>), dim3(p.blocks), threads, lds, st, a);
    else hipLaunchKernelGGL((em_fwd_kernel<T, 0, kEmLanes>), dim3(p.blocks), threads, lds, st, a);
  });
  RET_LAUNCH();
}

extern "C" int rtsds_entropy_finish(const void* wsp, size_t ws_bytes, int n, int h, int w, double coef, float* loss,
                                    float* mean_entropy, void* stream) {
  if (!loss || !mean_entropy || !em_shape_ok(n, h, w, 2) || !std::isfinite(coef)) return RTSDS_ERR_SHAPE;
  if (((uintptr_t)wsp & 15) || ((uintptr_t)loss & 3) || ((uintptr_t)mean_entropy & 3)) return RTSDS_ERR_UNSUPPORTED;
  const EmPlan p = em_plan(n, h, w, 2);
  if (!wsp || ws_bytes < (size_t)p.blocks * 2 * sizeof(float)) return RTSDS_ERR_WORKSPACE;
  hipLaunchKernelGGL(rs_finish_kernel<2>, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)wsp, p.blocks, coef,
                     RsOuts<2>{{loss, mean_entropy}});
  RET_LAUNCH();
}

extern "C" int rtsds_entropy_bwd(const void* wsp, size_t ws_bytes, const float* grad_loss, double coef_g, void* dx, int dtype, int n,
                                 int h, int w, int c, void* stream) {
  if (!grad_loss || !dx || !em_shape_ok(n, h, w, c) || !std::isfinite(coef_g)) return RTSDS_ERR_SHAPE;
  if (!em_dtype_ok(dtype) || ((uintptr_t)dx % em_elem(dtype)) || ((uintptr_t)wsp & 15) || ((uintptr_t)grad_loss & 3))
    return RTSDS_ERR_UNSUPPORTED;
  if (!wsp || ws_bytes < rtsds_entropy_workspace(n, h, w, c)) return RTSDS_ERR_WORKSPACE;
  const EmPlan p = em_plan(n, h, w, c);
  const float* term = (const float*)((const char*)wsp + p.part_bytes);
  const long total = (long)n * h * w * c;
  hipStream_t st = (hipStream_t)stream;
  DISPATCH_T(dtype, hipLaunchKernelGGL(rs_bwd_kernel<T>, dim3(ew_blocks(total / VecT<T>::N + 2)), dim3(256), 0, st, term, grad_loss,
                                       coef_g, (T*)dx, total));
  RET_LAUNCH();
}
