// BatchNorm2d (train: batch statistics; eval: running statistics) over NHWC [rows][c],
// fused with an optional residual add and ReLU / LeakyReLU, plus its backward.
//
// Statistics are single-pass: each thread keeps shifted sums (shift = its first sample) for
// its channels, which are merged across threads / blocks with Chan's parallel formula, so
// large-mean conv outputs (the reference feeds 0-255-scale normalised images,
// main.py:69-72) do not cancel catastrophically.  Three launches per direction:
// partial statistics (grid over row chunks) -> per-channel finalize -> vectorised apply.
#include "bn_dev.h"
#include "chan_dev.h"
#include <type_traits>
#include <algorithm>

static const int kBnMaxRB = 2048;  // row blocks of the partial-statistics pass
static const int kBnTinyRows = 64;  // up to this many rows: one block per channel finalizes and applies

// Threads of a 256-block are laid out [row group][channel vector]; TPR = threads per row.
// Host and device: the launch planning (bn_need) divides the rows by the kernels' own arithmetic.
template <int VEC> struct BnLayout {
  int tpr, rpi;  // threads per row, rows per block iteration
  __host__ __device__ BnLayout(int c) {
    tpr = (c + VEC - 1) / VEC;
    if (tpr > 256) tpr = 256;
    rpi = 256 / tpr;
  }
};
// A thread's place in grid (row blocks, blocks of 256 * VEC channels): channel vector cv of row
// group rg; channels ch0 .. ch0 + VEC - 1, of which cvalid exist; rows row0(), row0() + step(), ...
template <int VEC> struct BnTile : BnLayout<VEC> {
  int cl, cv, rg, ch0, cvalid;  // cl: channels of this block
  bool col, active;             // col: the channel vector exists; active: its row group too
  RT_DEV static int block_channels(int c) { return min(c - (int)blockIdx.y * 256 * VEC, 256 * VEC); }
  RT_DEV BnTile(int c) : BnLayout<VEC>(block_channels(c)) {
    cl = block_channels(c);
    cv = threadIdx.x % this->tpr;
    rg = threadIdx.x / this->tpr;
    ch0 = blockIdx.y * 256 * VEC + cv * VEC;
    cvalid = c - ch0;
    col = cv * VEC < cl;
    active = rg < this->rpi && col;
  }
  RT_DEV long row0() const { return (long)blockIdx.x * this->rpi + rg; }
  RT_DEV long step() const { return (long)gridDim.x * this->rpi; }
};

// scale/shift of y = x*scale + shift.  Written with explicit fma so the backward can
// recompute exactly the forward's pre-activation (ReLU mask without reading y).
RT_DEV void bn_coef(float g, float b, float m, float inv, float& sc, float& sh) {
  sc = g * inv;
  sh = fmaf(-m, sc, b);
}

RT_DEV void chan_merge(float& na, float& ma, float& Ma, float nb, float mb, float Mb) {
  if (nb == 0.f) return;
  if (na == 0.f) { na = nb; ma = mb; Ma = Mb; return; }
  const float n = na + nb, d = mb - ma;
  ma += d * (nb / n);
  Ma += Mb + d * d * (na * nb / n);
  na = n;
}

// Pass 1 (forward): part[(ch * RB + rb) * 4 + {0,1,2}] = (count, mean, M2) of block rb (16-B
// records: one vector store / load each)
// (channel-major: the finalize reads one contiguous run per channel).
template <typename T, int VEC>
__global__ void __launch_bounds__(256) bn_stats_kernel(const T* __restrict__ x, float* __restrict__ part, long rows, int c) {
  __shared__ float sh[3][256][VEC];
  const BnTile<VEC> t(c);
  const int tid = threadIdx.x, ch0 = t.ch0;
  float cnt = 0.f, shift[VEC], s1[VEC], s2[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { shift[j] = 0.f; s1[j] = 0.f; s2[j] = 0.f; }
  if (t.active) {
    long r = t.row0();
    const long step = t.step();
    if (r < rows) {
      load_vec<T, VEC>(x + r * c + ch0, shift, t.cvalid);
      cnt = 1.f;
      r += step;
    }
    for (; r < rows; r += step) {
      float v[VEC];
      load_vec<T, VEC>(x + r * c + ch0, v, t.cvalid);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const float d = v[j] - shift[j];
        s1[j] += d;
        s2[j] = fmaf(d, d, s2[j]);
      }
      cnt += 1.f;
    }
  }
  // thread-level (count, mean, M2)
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const float mean = cnt > 0.f ? shift[j] + s1[j] / cnt : 0.f;
    const float m2 = cnt > 0.f ? s2[j] - s1[j] * s1[j] / cnt : 0.f;
    sh[0][tid][j] = cnt;
    sh[1][tid][j] = mean;
    sh[2][tid][j] = fmaxf(m2, 0.f);
  }
  __syncthreads();
  if (t.rg == 0 && t.col) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float n = sh[0][tid][j], m = sh[1][tid][j], M = sh[2][tid][j];
      for (int g = 1; g < t.rpi; ++g) {
        const int o = g * t.tpr + t.cv;
        chan_merge(n, m, M, sh[0][o][j], sh[1][o][j], sh[2][o][j]);
      }
      if (ch0 + j < c) {
        *(f32x4*)(part + ((long)(ch0 + j) * gridDim.x + blockIdx.x) * 4) = f32x4{n, m, M, 0.f};
      }
    }
  }
}


// Pass 2 (forward): one wave per channel merges the row-block partials (Chan, lane-strided,
// then a shuffle tree), updates running stats and emits scale/shift.
RT_DEV void chan_merge_shfl(float& n, float& m, float& M) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float nb = __shfl_xor(n, o, 64), mb = __shfl_xor(m, o, 64), Mb = __shfl_xor(M, o, 64);
    chan_merge(n, m, M, nb, mb, Mb);
  }
}
// 4 waves per channel: wave w merges partials b = w*64 + lane (+ 256 k), then the four wave
// results are merged in wave order -- up to kBnMaxRB partials without a pre-merge launch.
// (returns true in thread 0, which then holds the channel's scale / shift in sc_out / sh_out)
RT_DEV bool bn_finalize_body(const float* __restrict__ part, int nrb, int c, long rows, const float* gamma, const float* beta,
                             float* rmean, float* rvar, float* smean, float* sinv, float* scale, float* shift, float momentum,
                             float eps, long long* nbt, float (*wr)[3], float& sc_out, float& sh_out) {
  const int ch = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (nbt && ch == 0 && threadIdx.x == 0) *nbt += 1;  // num_batches_tracked.add_(1)
  // the per-channel operands of the tail, loaded up front (in flight with the partials: the
  // tail then pays no extra memory round trip; thread 0 alone reads and writes them)
  float g0 = 1.f, b0 = 0.f, rm0 = 0.f, rv0 = 0.f;
  if (threadIdx.x == 0) {
    if (gamma) g0 = gamma[ch];
    if (beta) b0 = beta[ch];
    if (rmean) rm0 = rmean[ch];
    if (rvar) rv0 = rvar[ch];
  }
  float n = 0.f, m = 0.f, M = 0.f;
  // up to 8 partials per thread loaded before any merge (one L2 round trip instead of eight);
  // merge order b = tid, tid + 256, ... as before
  for (int b0 = threadIdx.x; b0 < nrb; b0 += 256 * 8) {
    float pn[8], pm[8], pM[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = min(b0 + 256 * u, nrb - 1);
      const f32x4 p = *(const f32x4*)(part + ((long)ch * nrb + b) * 4);  // clamped: unconditional
      pn[u] = b0 + 256 * u < nrb ? p[0] : 0.f;                             // zero count past nrb
      pm[u] = p[1];
      pM[u] = p[2];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) chan_merge(n, m, M, pn[u], pm[u], pM[u]);
  }
  chan_merge_shfl(n, m, M);
  if (lane == 0) { wr[wave][0] = n; wr[wave][1] = m; wr[wave][2] = M; }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  n = wr[0][0]; m = wr[0][1]; M = wr[0][2];
  for (int w = 1; w < 4; ++w) chan_merge(n, m, M, wr[w][0], wr[w][1], wr[w][2]);
  const float var = M / (float)rows;
  const float inv = 1.0f / sqrtf(var + eps);
  smean[ch] = m;
  sinv[ch] = inv;
  if (rmean) rmean[ch] = (1.f - momentum) * rm0 + momentum * m;
  if (rvar) {
    const float unb = rows > 1 ? M / (float)(rows - 1) : var;
    rvar[ch] = (1.f - momentum) * rv0 + momentum * unb;
  }
  bn_coef(g0, b0, m, inv, sc_out, sh_out);
  scale[ch] = sc_out;
  shift[ch] = sh_out;
  return true;
}
__global__ void __launch_bounds__(256) bn_finalize_kernel(const float* __restrict__ part, int nrb, int c, long rows, const float* gamma,
                                   const float* beta, float* rmean, float* rvar, float* smean, float* sinv,
                                   float* scale, float* shift, float momentum, float eps, long long* nbt) {
  __shared__ float wr[4][3];
  float sc, sh;
  bn_finalize_body(part, nrb, c, rows, gamma, beta, rmean, rvar, smean, sinv, scale, shift, momentum, eps, nbt, wr, sc, sh);
}
// The forward finalizes of a residual block's two BatchNorms (bn2 / bn3 and the downsample's, on
// tensors of one [rows][c] shape) in one launch: blockIdx.y picks the BatchNorm.
struct BnFin {
  const float* part;
  int nrb;
  const float *gamma, *beta;
  float *rmean, *rvar, *smean, *sinv, *scale, *shift;
  float momentum, eps;
  long long* nbt;
};
__global__ void __launch_bounds__(256) bn_finalize_pair_kernel(BnFin fa, BnFin fb, int c, long rows) {
  __shared__ float wr[4][3];
  const BnFin f = blockIdx.y ? fb : fa;
  float sc, sh;
  bn_finalize_body(f.part, f.nrb, c, rows, f.gamma, f.beta, f.rmean, f.rvar, f.smean, f.sinv, f.scale, f.shift, f.momentum, f.eps,
                   f.nbt, wr, sc, sh);
}
__global__ void bn_eval_coef_kernel(int c, const float* gamma, const float* beta, const float* rmean, const float* rvar,
                                    float* scale, float* shift, float* smean, float* sinv, float eps) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch >= c) return;
  const float inv = 1.0f / sqrtf(rvar[ch] + eps);
  if (smean) smean[ch] = rmean[ch];
  if (sinv) sinv[ch] = inv;
  const float g = gamma ? gamma[ch] : 1.f, b = beta ? beta[ch] : 0.f;
  bn_coef(g, b, rmean[ch], inv, scale[ch], shift[ch]);
}

RT_DEV float act_f(float v, int act) {
  if (act == RTSDS_ACT_RELU) return fmaxf(v, 0.f);
  if (act == RTSDS_ACT_LEAKY) return v > 0.f ? v : 0.2f * v;
  if (act == RTSDS_ACT_SIGMOID) return 1.f / (1.f + expf(-v));
  return v;
}
// Per-channel coefficients for a thread's VEC channels.  Coefficient arrays live in the
// 256-B aligned workspace and VEC > 1 only when c % VEC == 0, so VEC % 4 == 0 loads are 16 B.
template <int VEC>
RT_DEV void load_coef(const float* __restrict__ p, int ch0, int c, float* v) {
  if constexpr (VEC % 4 == 0) {
#pragma unroll
    for (int q = 0; q < VEC / 4; ++q) {
      const f32x4 t = *(const f32x4*)(p + ch0 + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * q + e] = t[e];
    }
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = p[min(ch0 + j, c - 1)];
  }
}

// Few rows (the attention modules' BatchNorms on [N, C] pooled rows): the finalize's block also
// applies y = act(x * scale + shift [+ res]) to its channel's rows (bn_apply_kernel's expression)
// -- one launch instead of two, bit-identical.
template <typename T>
__global__ void __launch_bounds__(256) bn_finalize_apply_kernel(const float* __restrict__ part, int nrb, int c, long rows,
                                                                 const float* gamma, const float* beta, float* rmean, float* rvar,
                                                                 float* smean, float* sinv, float* scale, float* shift,
                                                                 float momentum, float eps, long long* nbt, const T* __restrict__ x,
                                                                 const T* __restrict__ res, T* __restrict__ y, long ldy, int act) {
  __shared__ float wr[4][3];
  __shared__ float cs[2];
  float sc, sh;
  if (bn_finalize_body(part, nrb, c, rows, gamma, beta, rmean, rvar, smean, sinv, scale, shift, momentum, eps, nbt, wr, sc, sh)) {
    cs[0] = sc;
    cs[1] = sh;
  }
  __syncthreads();
  const int ch = blockIdx.x;
  for (long r = threadIdx.x; r < rows; r += 256) {
    float a = fmaf(to_f(x[r * c + ch]), cs[0], cs[1]);
    if (res) a += to_f(res[r * c + ch]);
    y[r * ldy + ch] = from_f<T>(act_f(a, act));
  }
}

// Pass 3 (forward): y = act(x * scale + shift [+ res]).  Same [row group][channel vector]
// layout as the statistics pass: each thread owns one channel vector for its whole row
// sweep, so the coefficients sit in registers and there is no per-element index division.
// ACT (here and in the backward passes): the activation fixed at compile time for the ones the
// networks use (RTSDS_ACT_NONE / RTSDS_ACT_RELU), < 0 = the runtime argument; with a runtime
// activation every element paid act_f's uniform compare-and-branch chain.
template <typename T, int VEC, int ACT>
__global__ void __launch_bounds__(256) bn_apply_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
                                                        const float* __restrict__ scale, const float* __restrict__ shift,
                                                        long rows, int c, int act_rt, long ldy) {
  const int act = ACT >= 0 ? ACT : act_rt;
  const BnTile<VEC> t(c);
  if (!t.active) return;
  float sc[VEC], sh[VEC];
  load_coef<VEC>(scale, t.ch0, c, sc);
  load_coef<VEC>(shift, t.ch0, c, sh);
  const int ch0 = t.ch0, cvalid = t.cvalid;
  const long step = t.step();
  long r = t.row0();
  // The row body stays written twice (two rows, then one): split into a load and a finish phase
  // per row, the compiler sinks the second row's loads behind the first row's wait whenever
  // there is a residual.
  for (; r + step < rows; r += 2 * step) {  // two independent rows in flight per thread
    float v0[VEC], v1[VEC], r0[VEC], r1[VEC];
    load_vec<T, VEC>(x + r * c + ch0, v0, cvalid);
    load_vec<T, VEC>(x + (r + step) * c + ch0, v1, cvalid);
    if (res) {
      load_vec<T, VEC>(res + r * c + ch0, r0, cvalid);
      load_vec<T, VEC>(res + (r + step) * c + ch0, r1, cvalid);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float a = fmaf(v0[j], sc[j], sh[j]), b = fmaf(v1[j], sc[j], sh[j]);
      if (res) { a += r0[j]; b += r1[j]; }
      v0[j] = act_f(a, act);
      v1[j] = act_f(b, act);
    }
    store_vec<T, VEC>(y + r * ldy + ch0, v0, cvalid);
    store_vec<T, VEC>(y + (r + step) * ldy + ch0, v1, cvalid);
  }
  if (r < rows) {
    float v0[VEC], r0[VEC];
    load_vec<T, VEC>(x + r * c + ch0, v0, cvalid);
    if (res) load_vec<T, VEC>(res + r * c + ch0, r0, cvalid);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      float a = fmaf(v0[j], sc[j], sh[j]);
      if (res) a += r0[j];
      v0[j] = act_f(a, act);
    }
    store_vec<T, VEC>(y + r * ldy + ch0, v0, cvalid);
  }
}

// Pass 3 (forward) of a training-mode residual BatchNorm + ReLU that keeps mask bits instead of y
// for its backward: bn_apply_kernel's y = relu(x * scale + shift + res) in its layout, and one byte
// per channel vector, bits[r][ch0 / VEC] = bn_y_bits of the values stored (c % VEC == 0).
// PAIR: res is the raw output of the block's downsample conv and scale2 / shift2 its BatchNorm's:
// the residual is round(res * scale2 + shift2), the value bn_apply_kernel<T, VEC, 0> would have
// stored as the skip tensor, which is never written.
template <typename T, int VEC, bool PAIR>
RT_DEV void bn_res_row(float* v, const float* rv, const float* sc, const float* sh, const float* sc2, const float* sh2) {
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    float r = rv[j];
    if constexpr (PAIR) r = to_f(from_f<T>(fmaf(r, sc2[j], sh2[j])));
    float a = fmaf(v[j], sc[j], sh[j]);
    a += r;
    v[j] = fmaxf(a, 0.f);
  }
}
template <typename T, int VEC, bool PAIR>
__global__ void __launch_bounds__(256) bn_apply_bits_kernel(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y,
                                                             uint8_t* __restrict__ bits, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, const float* __restrict__ scale2,
                                                             const float* __restrict__ shift2, long rows, int c) {
  static_assert(VEC == VecT<T>::N, "whole 16-byte channel vectors");
  const BnTile<VEC> t(c);
  if (!t.active) return;
  float sc[VEC], sh[VEC], sc2[PAIR ? VEC : 1], sh2[PAIR ? VEC : 1];
  load_coef<VEC>(scale, t.ch0, c, sc);
  load_coef<VEC>(shift, t.ch0, c, sh);
  if constexpr (PAIR) {
    load_coef<VEC>(scale2, t.ch0, c, sc2);
    load_coef<VEC>(shift2, t.ch0, c, sh2);
  }
  const int ch0 = t.ch0, cvalid = t.cvalid;
  const long step = t.step(), nv = c / VEC, bv = ch0 / VEC;
  long r = t.row0();
  for (; r + step < rows; r += 2 * step) {  // two independent rows in flight per thread, as bn_apply_kernel
    float v0[VEC], v1[VEC], r0[VEC], r1[VEC];
    load_vec<T, VEC>(x + r * c + ch0, v0, cvalid);
    load_vec<T, VEC>(x + (r + step) * c + ch0, v1, cvalid);
    load_vec<T, VEC>(res + r * c + ch0, r0, cvalid);
    load_vec<T, VEC>(res + (r + step) * c + ch0, r1, cvalid);
    bn_res_row<T, VEC, PAIR>(v0, r0, sc, sh, sc2, sh2);
    bn_res_row<T, VEC, PAIR>(v1, r1, sc, sh, sc2, sh2);
    store_vec<T, VEC>(y + r * c + ch0, v0, cvalid);
    store_vec<T, VEC>(y + (r + step) * c + ch0, v1, cvalid);
    bits[r * nv + bv] = (uint8_t)bn_y_bits<T, VEC>(v0);
    bits[(r + step) * nv + bv] = (uint8_t)bn_y_bits<T, VEC>(v1);
  }
  if (r < rows) {
    float v0[VEC], r0[VEC];
    load_vec<T, VEC>(x + r * c + ch0, v0, cvalid);
    load_vec<T, VEC>(res + r * c + ch0, r0, cvalid);
    bn_res_row<T, VEC, PAIR>(v0, r0, sc, sh, sc2, sh2);
    store_vec<T, VEC>(y + r * c + ch0, v0, cvalid);
    bits[r * nv + bv] = (uint8_t)bn_y_bits<T, VEC>(v0);
  }
}

// Pass 3 (forward) for a feature that is pooled next (the FeatureFusionModule's ConvBlock, whose
// output feeds a global average pool): y = act(x * scale + shift), bn_apply_kernel's expression,
// in chan_part_kernel<T, 1, false>'s partition, thread layout and order, which also leaves that
// kernel's per-slice sums of the rounded values -- bit for bit the two launches' results.
template <typename T>
struct BnApplyLoad {
  const T* x;
  T* y;
  float sc, sh;
  int act;
  RT_DEV float at(long o) const {
    const T v = from_f<T>(act_f(fmaf(to_f(x[o]), sc, sh), act));
    y[o] = v;
    return to_f(v);
  }
};
template <typename T>
__global__ void __launch_bounds__(256) bn_apply_gap_kernel(const T* __restrict__ x, T* __restrict__ y, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, float* __restrict__ part, long hw, int c,
                                                            int act) {
  __shared__ float red[256];
  const int ch = threadIdx.x % c;  // (c <= 256: the thread's channel in chan_part_body)
  chan_part_body<T, 1, false>(BnApplyLoad<T>{x, y, scale[ch], shift[ch], act}, (const T*)nullptr, part, hw, c, red);
}

// Where the backward passes read g (before the activation mask): the stored dY, or -- for a
// BatchNorm + ReLU feeding a 3x3 stride-2 max pool (the ResNet stem, fused forward in
// bn_relu_pool_fwd_kernel) -- a gather of the pooled gradient: input pixel r of channel vector
// ch0 receives dY_pool[o] from each of the <= 2 x 2 windows o covering it whose argmax byte
// names r.  The dY of the BatchNorm never exists in memory.
template <typename T>
struct GradDirect {
  static constexpr bool kDirect = true;
  const T* dy;
  int c;
  template <int VEC> RT_DEV void load(long r, int ch0, float* g, int cvalid) const { load_vec<T, VEC>(dy + r * c + ch0, g, cvalid); }
};
template <typename T>
struct GradPool {
  static constexpr bool kDirect = false;
  const T* dyp;
  const uint8_t* idx;
  int c, h, w, ho, wo, p;
  FastDiv f_w, f_h;
  template <int VEC> RT_DEV void load(long r, int ch0, float* g, int cvalid) const {
    static_assert(VEC == 8 && sizeof(T) == 2, "pooled gradient source: bf16 vectors of 8 channels");
    typedef typename VecT<T>::v16 V16;
    const uint32_t q = fdiv((uint32_t)r, f_w), img = fdiv(q, f_h);
    const int iw = (int)((uint32_t)r - q * w), ih = (int)(q - img * h);
    const int oh_lo = max(0, (ih + p - 1) / 2), ow_lo = max(0, (iw + p - 1) / 2);
    V16 gv[4];
    unsigned long long ib[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {  // clamped, unconditional (all in flight together)
      const int oh = min(oh_lo + (t >> 1), ho - 1), ow = min(ow_lo + (t & 1), wo - 1);
      const long o = (((long)img * ho + oh) * wo + ow) * c + ch0;
      gv[t] = *(const V16*)(dyp + o);
      ib[t] = *(const unsigned long long*)(idx + o);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) g[j] = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int oh = oh_lo + (t >> 1), ow = ow_lo + (t & 1);
      const int a = ih - (oh * 2 - p), b = iw - (ow * 2 - p);
      if (oh >= ho || ow >= wo || a < 0 || a >= 3 || b < 0 || b >= 3) continue;
      const unsigned want = (unsigned)(a * 3 + b);
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (((ib[t] >> (8 * j)) & 0xff) == want) g[j] += to_f(gv[t][j]);
    }
  }
};

// The FeatureFusionModule's feature gradient, never stored (rtsds_bn_bwd_ffm): the feature has two
// readers, the channel scale r = f * a + f and the global average pool, so its gradient is
// round(round(dr * (a + 1)) + round(dpooled / hw)) -- chscale_bwd_dx_kernel (mode 1) followed by
// gap_bwd_kernel's accumulate, the expressions and roundings of functional.GradJoin's order.
template <typename T>
struct GradScalePool {
  static constexpr bool kDirect = false;
  const T *dr, *att, *dp;  // [rows][c], [n][c], [n][c]
  int c;
  long hw;
  float inv;  // 1 / hw
  template <int VEC> RT_DEV void load(long r, int ch0, float* g, int cvalid) const {
    static_assert(VEC == 1, "scale + pool gradient source: narrow class maps, one channel per thread");
    if (cvalid <= 0) { g[0] = 0.f; return; }
    const long v = (r / hw) * c + ch0;
    const T s = from_f<T>(to_f(dr[r * c + ch0]) * (to_f(att[v]) + 1.f));
    const T p = from_f<T>(to_f(dp[v]) * inv);
    g[0] = to_f(from_f<T>(to_f(s) + to_f(p)));
  }
};

template <int VEC>
RT_DEV void bn_bwd_coef(int ch0, int c, const float* gamma, const float* beta, const float* mean, const float* sinv,
                        BnDx<VEC>& k) {
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const int ch = min(ch0 + j, c - 1);
    k.mu[j] = mean[ch];
    bn_coef(gamma ? gamma[ch] : 1.f, beta ? beta[ch] : 0.f, k.mu[j], sinv[ch], k.sc[j], k.sh[j]);
  }
}

// The backward statistics loop over the rows r0, r0 + step, ... of a thread's channel vector:
// sg += g, sgx += g * (x - mean), with g = dy * act'(.) (bn_mask).  kBnU rows are in flight per
// thread (loads issued before any use).  gout (HAS_Y, may be null): g is also stored.  g_last /
// xv_last (may be null): receive the last iteration's masked g and its x (rows past the end:
// g = 0), for a caller that applies from registers.
// YBITS (HAS_Y): the mask comes from ybits ([rows][c / VEC] bytes, bn_y_bits) instead of y.
// PAIR: the same g also feeds a second BatchNorm on x2 (the downsample BatchNorm of a residual
// block, whose incoming gradient is g): sgx2 += g * (x2 - mu2), in the same row order (its sum of
// g is sg).
constexpr int kBnU = 2;
template <typename T, int VEC, bool HAS_Y, class GS, bool YBITS = false, bool PAIR = false>
RT_DEV void bn_bwd_sums(const GS& gs, const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ gout, long r0,
                        long step, long rows, int c, const BnTile<VEC>& t, const BnDx<VEC>& k, int act, float* sg,
                        float* sgx, float (*g_last)[VEC], float (*xv_last)[VEC], const uint8_t* __restrict__ ybits = nullptr,
                        const T* __restrict__ x2 = nullptr, const float* mu2 = nullptr, float* sgx2 = nullptr) {
  static_assert(HAS_Y || !YBITS, "mask bits stand in for y");
  const int ch0 = t.ch0;
  for (long r = r0; r < rows; r += kBnU * step) {
    // (loop-local: arrays owned by the caller cost bn_bwd_stats_kernel registers)
    float g[kBnU][VEC], xv[kBnU][VEC], yv[HAS_Y ? kBnU : 1][VEC], x2v[PAIR ? kBnU : 1][VEC];
    unsigned yb[YBITS ? kBnU : 1];
#pragma unroll
    for (int u = 0; u < kBnU; ++u) {
      // clamped, unconditional loads (all rows in flight together); rows past the end
      // contribute g = 0
      const long rr = min(r + u * step, rows - 1);
      gs.template load<VEC>(rr, ch0, g[u], t.cvalid);
      load_vec<T, VEC>(x + rr * c + ch0, xv[u], t.cvalid);
      if constexpr (YBITS) yb[u] = ybits[rr * (c / VEC) + ch0 / VEC];
      else if constexpr (HAS_Y) load_vec<T, VEC>(y + rr * c + ch0, yv[u], t.cvalid);
      if constexpr (PAIR) load_vec<T, VEC>(x2 + rr * c + ch0, x2v[u], t.cvalid);
    }
#pragma unroll
    for (int u = 0; u < kBnU; ++u)
      if (r + u * step >= rows) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) g[u][j] = 0.f;
      }
#pragma unroll
    for (int u = 0; u < kBnU; ++u) {
      if constexpr (YBITS) bn_bits_y<VEC>(yb[u], yv[u]);
      bn_mask<VEC, HAS_Y>(g[u], yv[HAS_Y ? u : 0], xv[u], k.sc, k.sh, act);
      if (HAS_Y && gout && r + u * step < rows) store_vec<T, VEC>(gout + (r + u * step) * c + ch0, g[u], t.cvalid);
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        sg[j] += g[u][j];
        sgx[j] = fmaf(g[u][j], xv[u][j] - k.mu[j], sgx[j]);
        if constexpr (PAIR) sgx2[j] = fmaf(g[u][j], x2v[u][j] - mu2[j], sgx2[j]);
        if (g_last) { g_last[u][j] = g[u][j]; xv_last[u][j] = xv[u][j]; }
      }
    }
  }
}

// Sums sg / sgx over the block's row groups, in place.  True in the threads that then hold their
// channel vector's block totals (the first row group's: threadIdx.x == cv).
template <int VEC>
RT_DEV bool bn_bwd_block_sum(const BnTile<VEC>& t, float (*red)[256][VEC], float* sg, float* sgx) {
  const int tid = threadIdx.x;
  if ((t.tpr & (t.tpr - 1)) == 0 && t.tpr <= 64) {
    // power-of-two row width: sum the wave's rows with xor shuffles (lanes l and l ^ (tpr << i)
    // hold the same channel vector), then the four wave sums through LDS -- a per-block tail of
    // a few hundred cycles instead of a serial LDS loop over all rpi rows.
    const int lane = tid & 63, wave = tid >> 6;
    for (int o = t.tpr; o < 64; o <<= 1) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        sg[j] += __shfl_xor(sg[j], o, 64);
        sgx[j] += __shfl_xor(sgx[j], o, 64);
      }
    }
    if (lane < t.tpr) {
#pragma unroll
      for (int j = 0; j < VEC; ++j) { red[0][wave * 64 + lane][j] = sg[j]; red[1][wave * 64 + lane][j] = sgx[j]; }
    }
    __syncthreads();
    if (tid >= t.tpr || tid * VEC >= t.cl) return false;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      sg[j] = (red[0][tid][j] + red[0][64 + tid][j]) + (red[0][128 + tid][j] + red[0][192 + tid][j]);
      sgx[j] = (red[1][tid][j] + red[1][64 + tid][j]) + (red[1][128 + tid][j] + red[1][192 + tid][j]);
    }
    return true;
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) { red[0][tid][j] = sg[j]; red[1][tid][j] = sgx[j]; }
  __syncthreads();
  if (t.rg != 0 || !t.col) return false;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    float a = red[0][tid][j], b = red[1][tid][j];
    for (int gi = 1; gi < t.rpi; ++gi) {
      a += red[0][gi * t.tpr + t.cv][j];
      b += red[1][gi * t.tpr + t.cv][j];
    }
    sg[j] = a;
    sgx[j] = b;
  }
  return true;
}

// The backward finalize of one channel: its operands, loaded up front (in flight with the
// partials, see bn_finalize_body), and the tail that turns the channel's (sum g, sum g*(x-mean))
// into dgamma, dbeta and the coefficients A, B, C of dx = A*g + B*(x-mean) + C.
struct BnBwdOps {
  float inv = 0.f, g = 1.f, bt = 0.f, mu = 0.f, dg0 = 0.f, db0 = 0.f;
};
RT_DEV BnBwdOps bn_bwd_ops(int ch, const float* gamma, const float* beta, const float* smean, const float* sinv,
                           const float* dgamma, const float* dbeta, int accumulate) {
  BnBwdOps o;
  o.inv = sinv[ch];
  o.mu = smean[ch];
  if (gamma) o.g = gamma[ch];
  if (beta) o.bt = beta[ch];
  if (accumulate && dgamma) o.dg0 = dgamma[ch];
  if (accumulate && dbeta) o.db0 = dbeta[ch];
  return o;
}
RT_DEV void bn_bwd_tail(const BnBwdOps& o, float sg, float sgx, int ch, long rows, int training, int accumulate,
                        float* dgamma, float* dbeta, float& A, float& B, float& C) {
  const float inv = o.inv;
  if (dgamma) dgamma[ch] = accumulate ? o.dg0 + sgx * inv : sgx * inv;
  if (dbeta) dbeta[ch] = accumulate ? o.db0 + sg : sg;
  const float a = o.g * inv;
  const float invn = 1.f / (float)rows;
  A = a;
  B = training ? -a * inv * inv * sgx * invn : 0.f;
  C = training ? -a * sg * invn : 0.f;
}
// ... and the six coefficient rows of the apply pass:
// coef = [A | B | C | mean | scale | shift] x c  (the last three for the mask recompute).
RT_DEV void bn_bwd_coef_rows(const BnBwdOps& o, float sg, float sgx, int ch, int c, long rows, int training, int accumulate,
                             float* dgamma, float* dbeta, float* coef) {
  bn_bwd_tail(o, sg, sgx, ch, rows, training, accumulate, dgamma, dbeta, coef[ch], coef[c + ch], coef[2 * c + ch]);
  coef[3 * c + ch] = o.mu;
  bn_coef(o.g, o.bt, o.mu, o.inv, coef[4 * c + ch], coef[5 * c + ch]);
}

// dx (in place of xv) and dres of one row from its masked g and x; off = r * c + ch0
template <typename T, int VEC>
RT_DEV void bn_bwd_row_store(T* __restrict__ dx, T* __restrict__ dres, long off, const BnDx<VEC>& k, int cvalid, const float* g,
                             float* xv) {
#pragma unroll
  for (int j = 0; j < VEC; ++j) xv[j] = bn_bwd_dx<VEC>(k, j, g[j], xv[j]);
  if (dx) store_vec<T, VEC>(dx + off, xv, cvalid);
  if (dres) store_vec<T, VEC>(dres + off, g, cvalid);
}
// One whole row r: load, mask, store.
template <typename T, int VEC, class GS>
RT_DEV void bn_bwd_row(const GS& gs, const T* __restrict__ x, const T* __restrict__ y, T* __restrict__ dx, T* __restrict__ dres,
                       long r, int c, const BnTile<VEC>& t, const BnDx<VEC>& k, int act) {
  const long off = r * c + t.ch0;
  float g[VEC], xv[VEC];
  gs.template load<VEC>(r, t.ch0, g, t.cvalid);
  load_vec<T, VEC>(x + off, xv, t.cvalid);
  bn_row_mask<T, VEC>(g, y ? y + off : nullptr, xv, k, act, t.cvalid);
  bn_bwd_row_store<T, VEC>(dx, dres, off, k, t.cvalid, g, xv);
}

// Backward pass 1: part[(rb*c+ch)*2 + {0,1}] = (sum g, sum g*(x-mean)) with g = dy*act'(y) --
// row-block-major, so each block's partials leave as contiguous stores (channel-major rows
// scattered 8-B stores RB*c*8 bytes apart: 16 MB of them for 1024 channels).  Merged by
// bn_bwd_finalize_rb_kernel.
// HAS_Y: the activation mask comes from y (residual BNs); otherwise from x (no y registers).
// gout (HAS_Y): g = dy * act'(y) is also stored (the residual branch's gradient, and the apply
// pass's input instead of dy and y).
template <typename T, int VEC, bool HAS_Y, class GS, int ACT>
__global__ void __launch_bounds__(256) bn_bwd_stats_kernel(const GS gs, const T* __restrict__ x,
                                                            const T* __restrict__ y, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ mean,
                                                            const float* __restrict__ sinv, float* __restrict__ part,
                                                            long rows, int c, int act_rt, T* __restrict__ gout) {
  const int act = ACT >= 0 ? ACT : act_rt;
  __shared__ float red[2][256][VEC];
  const BnTile<VEC> t(c);
  BnDx<VEC> k;
  float sg[VEC], sgx[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { sg[j] = 0.f; sgx[j] = 0.f; }
  if (t.active) {
    bn_bwd_coef<VEC>(t.ch0, c, gamma, beta, mean, sinv, k);
    bn_bwd_sums<T, VEC, HAS_Y>(gs, x, y, gout, t.row0(), t.step(), rows, c, t, k, act, sg, sgx, nullptr, nullptr);
  }
  if (!bn_bwd_block_sum<VEC>(t, red, sg, sgx)) return;
#pragma unroll
  for (int j = 0; j < VEC; ++j)
    if (t.ch0 + j < c) *(float2*)(part + ((long)blockIdx.x * c + t.ch0 + j) * 2) = make_float2(sg[j], sgx[j]);
}

// bn_bwd_stats_kernel<T, VEC, true, GS, RTSDS_ACT_RELU> with the mask read from the forward's bits
// (bn_apply_bits_kernel) instead of y: the same g, gout store and partials from one byte per
// channel vector in place of a 16-byte read.
// PAIR: g is also the incoming gradient of the block's downsample BatchNorm (no activation) on x2:
// part2 receives the partials bn_bwd_stats_kernel<T, VEC, false, GradDirect<T>, 0> forms from the
// stored g -- the same sum of g, and sum g * (x2 - mean2) in the same order.  g is exactly dy or
// dy * 0, so the pair's apply pass re-forms it from dy and the bits and gout is not needed.
template <typename T, int VEC, class GS, bool PAIR>
__global__ void __launch_bounds__(256) bn_bwd_stats_bits_kernel(const GS gs, const T* __restrict__ x,
                                                                 const uint8_t* __restrict__ bits, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, const float* __restrict__ mean,
                                                                 const float* __restrict__ sinv, float* __restrict__ part,
                                                                 long rows, int c, T* __restrict__ gout,
                                                                 const T* __restrict__ x2, const float* __restrict__ mean2,
                                                                 float* __restrict__ part2) {
  __shared__ float red[2][256][VEC];
  const BnTile<VEC> t(c);
  BnDx<VEC> k;
  float sg[VEC], sgx[VEC], sg2[PAIR ? VEC : 1], sgx2[PAIR ? VEC : 1], mu2[PAIR ? VEC : 1];
#pragma unroll
  for (int j = 0; j < VEC; ++j) { sg[j] = 0.f; sgx[j] = 0.f; }
  if constexpr (PAIR) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) { sgx2[j] = 0.f; mu2[j] = mean2[min(t.ch0 + j, c - 1)]; }
  }
  if (t.active) {
    bn_bwd_coef<VEC>(t.ch0, c, gamma, beta, mean, sinv, k);
    bn_bwd_sums<T, VEC, true, GS, true, PAIR>(gs, x, (const T*)nullptr, gout, t.row0(), t.step(), rows, c, t, k, RTSDS_ACT_RELU, sg,
                                              sgx, nullptr, nullptr, bits, x2, mu2, sgx2);
  }
  if constexpr (PAIR) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) sg2[j] = sg[j];
  }
  const bool owner = bn_bwd_block_sum<VEC>(t, red, sg, sgx);
  if (owner) {
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (t.ch0 + j < c) *(float2*)(part + ((long)blockIdx.x * c + t.ch0 + j) * 2) = make_float2(sg[j], sgx[j]);
  }
  if constexpr (PAIR) {
    __syncthreads();  // red is reused
    if (!bn_bwd_block_sum<VEC>(t, red, sg2, sgx2)) return;
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (t.ch0 + j < c) *(float2*)(part2 + ((long)blockIdx.x * c + t.ch0 + j) * 2) = make_float2(sg2[j], sgx2[j]);
  }
}

// All three backward passes in one launch when the statistics pass has a single row block
// (bn_bwd_rb == 1: the attention modules' BatchNorms on [N, C] pooled rows): the same statistics
// loop and reduction as bn_bwd_stats_kernel (grid (1, channel blocks)), the finalize of a single
// partial (bn_bwd_finalize_rb_kernel's 0 + p), the apply of bn_bwd_apply_kernel -- so the results
// are bit-identical to the three launches.
template <typename T, int VEC, bool HAS_Y, class GS, int ACT>
__global__ void __launch_bounds__(256) bn_bwd_tiny_kernel(const GS gs, const T* __restrict__ x, const T* __restrict__ y,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ mean, const float* __restrict__ sinv,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, T* __restrict__ dx,
                                                           T* __restrict__ dres, long rows, int c, int act_rt, int training,
                                                           int accumulate) {
  const int act = ACT >= 0 ? ACT : act_rt;
  __shared__ float red[2][256][VEC];
  __shared__ float cf[3][256 * VEC];
  const BnTile<VEC> t(c);
  // rows <= kBnU * rpi: the statistics loop runs once and its (masked) g and x stay in registers
  // for the apply -- one memory round trip fewer
  const bool one_pass = rows <= kBnU * (long)t.rpi;
  BnDx<VEC> k;
  float sg[VEC], sgx[VEC], g[kBnU][VEC], xv[kBnU][VEC];
  BnBwdOps ops[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    sg[j] = 0.f;
    sgx[j] = 0.f;
    ops[j] = bn_bwd_ops(min(t.ch0 + j, c - 1), gamma, beta, mean, sinv, dgamma, dbeta, accumulate);
  }
  if (t.active) {
    bn_bwd_coef<VEC>(t.ch0, c, gamma, beta, mean, sinv, k);
    bn_bwd_sums<T, VEC, HAS_Y>(gs, x, y, (T*)nullptr, t.rg, t.rpi, rows, c, t, k, act, sg, sgx, g, xv);  // (one row block)
  }
  if (bn_bwd_block_sum<VEC>(t, red, sg, sgx)) {
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const int ch = t.ch0 + j, o = t.cv * VEC + j;
      if (ch >= c) continue;
      // 0 + p: bn_bwd_finalize_rb_kernel's sum of one partial
      bn_bwd_tail(ops[j], 0.f + sg[j], 0.f + sgx[j], ch, rows, training, accumulate, dgamma, dbeta, cf[0][o], cf[1][o],
                  cf[2][o]);
    }
  }
  __syncthreads();
  if (!t.active || (!dx && !dres)) return;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    k.a[j] = cf[0][t.cv * VEC + j];
    k.b[j] = cf[1][t.cv * VEC + j];
    k.k[j] = cf[2][t.cv * VEC + j];
  }
  if (one_pass) {
#pragma unroll
    for (int u = 0; u < kBnU; ++u) {
      const long r = t.rg + u * (long)t.rpi, off = r * c + t.ch0;
      if (r < rows) bn_bwd_row_store<T, VEC>(dx, dres, off, k, t.cvalid, g[u], xv[u]);
    }
    return;
  }
  for (long r = t.rg; r < rows; r += t.rpi) bn_bwd_row<T, VEC>(gs, x, HAS_Y ? y : (const T*)nullptr, dx, dres, r, c, t, k, act);
}

// Backward pass 2: coefficients  dx = A*g + B*(x-mean) + C  per channel (one wave each).
// coef = [A | B | C | mean | scale | shift] x c  (the last three for the mask recompute).
__global__ void __launch_bounds__(256) bn_bwd_finalize_kernel(const float* __restrict__ part, int nrb, int c, long rows, const float* gamma,
                                       const float* beta, const float* smean, const float* sinv, float* dgamma, float* dbeta,
                                       float* coef, int training, int accumulate) {
  __shared__ float wr[4][2];
  const int ch = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  BnBwdOps ops;  // (thread 0 alone reads and writes the channel's operands)
  if (threadIdx.x == 0) ops = bn_bwd_ops(ch, gamma, beta, smean, sinv, dgamma, dbeta, accumulate);
  float sg = 0.f, sgx = 0.f;
  for (int b0 = threadIdx.x; b0 < nrb; b0 += 256 * 8) {  // 8 partials in flight per thread
    float pg[8], px[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = min(b0 + 256 * u, nrb - 1);
      const bool ok = b0 + 256 * u < nrb;
      const float2 pr = *(const float2*)(part + ((long)ch * nrb + b) * 2);
      const float g = pr.x, gx = pr.y;
      pg[u] = ok ? g : 0.f;
      px[u] = ok ? gx : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) { sg += pg[u]; sgx += px[u]; }
  }
  sg = wave_sum(sg);
  sgx = wave_sum(sgx);
  if (lane == 0) { wr[wave][0] = sg; wr[wave][1] = sgx; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  sg = (wr[0][0] + wr[1][0]) + (wr[2][0] + wr[3][0]);
  sgx = (wr[0][1] + wr[1][1]) + (wr[2][1] + wr[3][1]);
  bn_bwd_coef_rows(ops, sg, sgx, ch, c, rows, training, accumulate, dgamma, dbeta, coef);
}

// Backward pass 2 for the row-block-major partials of bn_bwd_stats_kernel: 16 channels per
// block, lane q (0..15) of a channel sums row blocks q, q + 16, ... (8 in flight, 128-B rows of
// 16 channels per load group), the 16 lane sums added in a fixed tree order; coefficients as
// bn_bwd_finalize_kernel.
RT_DEV void bn_bwd_finalize_rb_body(const float* __restrict__ part, int nrb, int c, long rows, const float* gamma,
                                    const float* beta, const float* smean, const float* sinv, float* dgamma, float* dbeta,
                                    float* coef, int training, int accumulate, float (*wr)[16][2]) {
  const int cl = threadIdx.x & 15, q = threadIdx.x >> 4, ch = blockIdx.x * 16 + cl;
  const int chc = min(ch, c - 1);
  BnBwdOps ops;
  if (q == 0) ops = bn_bwd_ops(chc, gamma, beta, smean, sinv, dgamma, dbeta, accumulate);
  float sg = 0.f, sgx = 0.f;
  for (int b0 = q; b0 < nrb; b0 += 16 * 8) {
    float2 pv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int b = min(b0 + 16 * u, nrb - 1);  // clamped: unconditional
      pv[u] = *(const float2*)(part + ((long)b * c + chc) * 2);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (b0 + 16 * u < nrb) { sg += pv[u].x; sgx += pv[u].y; }
  }
  wr[q][cl][0] = sg;
  wr[q][cl][1] = sgx;
  __syncthreads();
  if (q != 0 || ch >= c) return;
  float t0[8], t1[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { t0[i] = wr[2 * i][cl][0] + wr[2 * i + 1][cl][0]; t1[i] = wr[2 * i][cl][1] + wr[2 * i + 1][cl][1]; }
#pragma unroll
  for (int i = 0; i < 4; ++i) { t0[i] = t0[2 * i] + t0[2 * i + 1]; t1[i] = t1[2 * i] + t1[2 * i + 1]; }
  sg = (t0[0] + t0[1]) + (t0[2] + t0[3]);
  sgx = (t1[0] + t1[1]) + (t1[2] + t1[3]);
  bn_bwd_coef_rows(ops, sg, sgx, ch, c, rows, training, accumulate, dgamma, dbeta, coef);
}
__global__ void __launch_bounds__(256) bn_bwd_finalize_rb_kernel(const float* __restrict__ part, int nrb, int c, long rows,
                                                                  const float* gamma, const float* beta, const float* smean,
                                                                  const float* sinv, float* dgamma, float* dbeta, float* coef,
                                                                  int training, int accumulate) {
  __shared__ float wr[16][16][2];
  bn_bwd_finalize_rb_body(part, nrb, c, rows, gamma, beta, smean, sinv, dgamma, dbeta, coef, training, accumulate, wr);
}
// The backward finalizes of a residual block's two BatchNorms (bn_bwd_stats_bits_kernel<PAIR>'s two
// partial sets) in one launch: blockIdx.y picks the BatchNorm, each runs bn_bwd_finalize_rb_kernel's
// body (training mode).
struct BnBwdFin {
  const float *part, *gamma, *beta, *smean, *sinv;
  float *dgamma, *dbeta, *coef;
  int accumulate;
};
__global__ void __launch_bounds__(256) bn_bwd_finalize_pair_kernel(BnBwdFin fa, BnBwdFin fb, int nrb, int c, long rows) {
  __shared__ float wr[16][16][2];
  const BnBwdFin f = blockIdx.y ? fb : fa;
  bn_bwd_finalize_rb_body(f.part, nrb, c, rows, f.gamma, f.beta, f.smean, f.sinv, f.dgamma, f.dbeta, f.coef, 1, f.accumulate, wr);
}

// Backward pass 3: dx = A*g + B*(x - mean) + C;  dres = g.  Layout as bn_apply_kernel.
template <typename T, int VEC, class GS, int ACT>
__global__ void __launch_bounds__(256) bn_bwd_apply_kernel(const GS gs, const T* __restrict__ x,
                                                            const T* __restrict__ y, T* __restrict__ dx, T* __restrict__ dres,
                                                            const float* __restrict__ coef, long rows, int c, int act_rt) {
  const int act = ACT >= 0 ? ACT : act_rt;
  const BnTile<VEC> t(c);
  if (!t.active) return;
  BnDx<VEC> k;
  load_coef<VEC>(coef, t.ch0, c, k.a);
  load_coef<VEC>(coef + c, t.ch0, c, k.b);
  load_coef<VEC>(coef + 2 * c, t.ch0, c, k.k);
  load_coef<VEC>(coef + 3 * c, t.ch0, c, k.mu);
  if (act && !y) {
    load_coef<VEC>(coef + 4 * c, t.ch0, c, k.sc);
    load_coef<VEC>(coef + 5 * c, t.ch0, c, k.sh);
  }
  const long step = t.step();
  long r = t.row0();
  const int ch0 = t.ch0, cvalid = t.cvalid;
  // (the row body written twice, as in bn_apply_kernel: phase by phase per row, the x loads of
  // the two rows wait for each other and the runtime-activation instantiations take 14 more
  // registers)
  for (; r + step < rows; r += 2 * step) {  // two independent rows in flight per thread
    const long o0 = r * c + ch0, o1 = o0 + step * c;
    float g0[VEC], x0[VEC], g1[VEC], x1[VEC];
    gs.template load<VEC>(r, ch0, g0, cvalid);
    load_vec<T, VEC>(x + o0, x0, cvalid);
    gs.template load<VEC>(r + step, ch0, g1, cvalid);
    load_vec<T, VEC>(x + o1, x1, cvalid);
    bn_row_mask<T, VEC>(g0, y ? y + o0 : nullptr, x0, k, act, cvalid);
    bn_row_mask<T, VEC>(g1, y ? y + o1 : nullptr, x1, k, act, cvalid);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      x0[j] = bn_bwd_dx<VEC>(k, j, g0[j], x0[j]);
      x1[j] = bn_bwd_dx<VEC>(k, j, g1[j], x1[j]);
    }
    if (dx) {
      store_vec<T, VEC>(dx + o0, x0, cvalid);
      store_vec<T, VEC>(dx + o1, x1, cvalid);
    }
    if (dres) {
      store_vec<T, VEC>(dres + o0, g0, cvalid);
      store_vec<T, VEC>(dres + o1, g1, cvalid);
    }
  }
  if (r < rows) bn_bwd_row<T, VEC>(gs, x, y, dx, dres, r, c, t, k, act);
}

// Backward pass 3 of a residual block's two BatchNorms: g = dy * relu'(y) re-formed from dy and
// the mask bits (the value the separate passes store and read back), then dxa = A*g + B*(xa - mean)
// + C with bn2's coefficients and dxb likewise with the downsample BatchNorm's -- the two
// bn_bwd_apply_kernel<T, VEC, GradDirect<T>, 0> launches from one read of g.
template <typename T, int VEC>
RT_DEV void bn_bwd_pair_row(T* __restrict__ dxa, T* __restrict__ dxb, long off, const BnDx<VEC>& ka, const BnDx<VEC>& kb,
                            int cvalid, unsigned yb, float* g, float* xa, float* xb) {
  float yv[VEC];
  bn_bits_y<VEC>(yb, yv);
  bn_mask<VEC, true>(g, yv, xa, ka.sc, ka.sh, RTSDS_ACT_RELU);
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    xa[j] = bn_bwd_dx<VEC>(ka, j, g[j], xa[j]);
    xb[j] = bn_bwd_dx<VEC>(kb, j, g[j], xb[j]);
  }
  store_vec<T, VEC>(dxa + off, xa, cvalid);
  store_vec<T, VEC>(dxb + off, xb, cvalid);
}
template <int VEC>
RT_DEV void bn_bwd_load_abk(const float* __restrict__ coef, int ch0, int c, BnDx<VEC>& k) {
  load_coef<VEC>(coef, ch0, c, k.a);
  load_coef<VEC>(coef + c, ch0, c, k.b);
  load_coef<VEC>(coef + 2 * c, ch0, c, k.k);
  load_coef<VEC>(coef + 3 * c, ch0, c, k.mu);
}
template <typename T, int VEC, class GS>
__global__ void __launch_bounds__(256) bn_bwd_apply_pair_kernel(const GS gs, const uint8_t* __restrict__ bits,
                                                                 const T* __restrict__ xa, const T* __restrict__ xb,
                                                                 T* __restrict__ dxa, T* __restrict__ dxb,
                                                                 const float* __restrict__ coefa, const float* __restrict__ coefb,
                                                                 long rows, int c) {
  const BnTile<VEC> t(c);
  if (!t.active) return;
  BnDx<VEC> ka, kb;
  bn_bwd_load_abk<VEC>(coefa, t.ch0, c, ka);
  bn_bwd_load_abk<VEC>(coefb, t.ch0, c, kb);
  const int ch0 = t.ch0, cvalid = t.cvalid;
  const long step = t.step(), nv = c / VEC, bv = ch0 / VEC;
  long r = t.row0();
  for (; r + step < rows; r += 2 * step) {  // two independent rows in flight per thread
    const long o0 = r * c + ch0, o1 = o0 + step * c;
    float g0[VEC], a0[VEC], b0[VEC], g1[VEC], a1[VEC], b1[VEC];
    gs.template load<VEC>(r, ch0, g0, cvalid);
    load_vec<T, VEC>(xa + o0, a0, cvalid);
    load_vec<T, VEC>(xb + o0, b0, cvalid);
    const unsigned y0 = bits[r * nv + bv];
    gs.template load<VEC>(r + step, ch0, g1, cvalid);
    load_vec<T, VEC>(xa + o1, a1, cvalid);
    load_vec<T, VEC>(xb + o1, b1, cvalid);
    const unsigned y1 = bits[(r + step) * nv + bv];
    bn_bwd_pair_row<T, VEC>(dxa, dxb, o0, ka, kb, cvalid, y0, g0, a0, b0);
    bn_bwd_pair_row<T, VEC>(dxa, dxb, o1, ka, kb, cvalid, y1, g1, a1, b1);
  }
  if (r < rows) {
    const long o0 = r * c + ch0;
    float g0[VEC], a0[VEC], b0[VEC];
    gs.template load<VEC>(r, ch0, g0, cvalid);
    load_vec<T, VEC>(xa + o0, a0, cvalid);
    load_vec<T, VEC>(xb + o0, b0, cvalid);
    bn_bwd_pair_row<T, VEC>(dxa, dxb, o0, ka, kb, cvalid, bits[r * nv + bv], g0, a0, b0);
  }
}

// ------------------------------------------------------------------ host
// f(std::integral_constant<int, A>) with A the compile-time activation variant of the kernels above
template <typename F>
static void with_act(int act, F f) {
  if (act == RTSDS_ACT_NONE) f(std::integral_constant<int, RTSDS_ACT_NONE>());
  else if (act == RTSDS_ACT_RELU) f(std::integral_constant<int, RTSDS_ACT_RELU>());
  else f(std::integral_constant<int, -1>());
}
// f(BnKind<T, VEC>) for the storage type and channel vector of (dtype, c)
template <typename T_, int VEC_> struct BnKind {
  typedef T_ T;
  static constexpr int VEC = VEC_;
};
template <typename F>
static int bn_dispatch(int dtype, int c, F f) {
  if (dtype == RTSDS_BF16) {
    if (c % 8 == 0) f(BnKind<bf16, 8>());
    else f(BnKind<bf16, 1>());
  } else if (dtype == RTSDS_F32) {
    if (c % 4 == 0) f(BnKind<float, 4>());
    else f(BnKind<float, 1>());
  } else return RTSDS_ERR_UNSUPPORTED;
  return RTSDS_OK;
}

// Row-block iterations that cover the rows (the kernels' own layout arithmetic)
template <int VEC>
static long bn_need(long rows, int c) {
  const BnLayout<VEC> L(c);
  return (rows + L.rpi - 1) / L.rpi;
}
// Row blocks of the reduction passes: enough to fill the chip (8+ waves per CU), at least
// 4 row-iterations per thread, at most kBnMaxRB partials to merge.
template <int VEC>
static int bn_rb(long rows, int c) {
  const long need = bn_need<VEC>(rows, c);
  long rb = std::min<long>(need, kBnMaxRB);
  rb = std::max<long>(1, std::min<long>(rb, (need + 7) / 8));
  return (int)rb;
}
// Row blocks of the elementwise passes: ~2 rows per thread.
static constexpr auto kBnApplyMaxRB = (1L << 24);
template <int VEC>
static int bn_apply_rb(long rows, int c) {
  const long need = bn_need<VEC>(rows, c);
  return (int)std::max<long>(1, std::min<long>((need + 1) / 2, kBnApplyMaxRB));
}
static constexpr auto kBnBwdRBMax = 512;
static constexpr auto kBnBwdRBDiv = 8;
// Row blocks of the backward statistics pass (row-block-major partials, merged 16 lanes per
// channel by bn_bwd_finalize_rb_kernel).  At most 512 (tools/ab_bn2.sh, stats pass: 33,540 x
// 1024 58.8 -> 29.2 us, 262,144 x 128 41.3 -> 27.7 us, 262,144 x 64 17.6 -> 15.6 us against 2048
// channel-major row blocks; finalize unchanged at ~5 us).
template <int VEC>
static int bn_bwd_rb(long rows, int c) {
  const long need = bn_need<VEC>(rows, c);
  long rb = std::min<long>(need, kBnBwdRBMax);
  rb = std::max<long>(1, std::min<long>(rb, (need + kBnBwdRBDiv - 1) / kBnBwdRBDiv));
  return (int)rb;
}
template <int VEC>
static dim3 bn_grid(int rb, int c) { return dim3(rb, rt_cdiv(c, 256 * VEC)); }

static size_t bn_part_floats(long rows, int c) { return (size_t)bn_rb<1>(rows, c) * c * 4; }

// Workspace: [row-block partials | 8 coefficient arrays], each part
// 256-B aligned (coefficient arrays are read with 16-B vector loads).
static size_t al64f(size_t n) { return (n + 63) & ~(size_t)63; }
struct BnWs {
  float *part, *coef;
};
static BnWs bn_ws(void* ws, long rows, int c) {
  BnWs w;
  w.part = (float*)ws;
  w.coef = w.part + al64f(bn_part_floats(rows, c));
  return w;
}
extern "C" size_t rtsds_bn_workspace(long rows, int c) {
  if (rows <= 0 || c <= 0) return 256;
  // partials (3 floats x RB x c; VEC=1 gives the most row blocks) + 8 x c
  return (al64f(bn_part_floats(rows, c)) + al64f((size_t)c * 8)) * 4 + 256;
}

// One BatchNorm call, either direction, as the entry points hand it to the launch functions.
struct BnArgs {
  long rows = 0;
  int c = 0, training = 0, act = 0, accumulate = 0;
  const void *x = nullptr, *res = nullptr, *dy = nullptr, *ykept = nullptr;  // ykept: the backward's mask source
  void *y = nullptr, *dx = nullptr, *dres = nullptr;                         // y: the forward's output
  long ldy = 0;                                                              // row pitch of y (forward) / dy (backward)
  const float *gamma = nullptr, *beta = nullptr;
  float *rmean = nullptr, *rvar = nullptr, *dgamma = nullptr, *dbeta = nullptr;
  float *smean = nullptr, *sinv = nullptr;  // written by the forward, read by the backward
  long long* nbt = nullptr;
  float momentum = 0.f, eps = 0.f;
  const float* pre = nullptr;  // partial statistics a conv epilogue already produced, pre_nrb per channel
  int pre_nrb = 0;
  bool coef_only = false;  // backward: statistics + finalize only, w.coef is the caller's buffer
  BnWs w = {nullptr, nullptr};
  hipStream_t st = nullptr;
  BnArgs(long rows_, int c_, void* ws, void* stream)
      : rows(rows_), c(c_), w(bn_ws(ws, rows_, c_)), st((hipStream_t)stream) {}
  void affine(const float* g, const float* b, const float* sm, const float* si) {
    gamma = g, beta = b, smean = const_cast<float*>(sm), sinv = const_cast<float*>(si);
  }
};

// The forward's prologue: scale | shift into the first two coefficient rows.  Training: the
// statistics pass (unless a conv epilogue produced the partials), then the finalize; eval: from the
// running statistics.  apply_too (training, few rows): the finalize's block also applies, and
// nothing is left to launch.
// The training forward's partial statistics: the conv epilogue's, else our own pass's (rb of them per channel)
template <typename T, int VEC>
static const float* bn_fwd_stats(const BnArgs& a, int& rb) {
  rb = a.pre_nrb;
  if (a.pre) return a.pre;
  rb = bn_rb<VEC>(a.rows, a.c);
  hipLaunchKernelGGL((bn_stats_kernel<T, VEC>), bn_grid<VEC>(rb, a.c), dim3(256), 0, a.st, (const T*)a.x, a.w.part, a.rows, a.c);
  return a.w.part;
}
template <typename T, int VEC>
static void bn_fwd_coefs(const BnArgs& a, bool apply_too = false) {
  const int c = a.c;
  float *scale = a.w.coef, *shift = a.w.coef + c;
  if (!a.training) {
    hipLaunchKernelGGL(bn_eval_coef_kernel, dim3(rt_cdiv(c, 256)), dim3(256), 0, a.st, c, a.gamma, a.beta, a.rmean, a.rvar, scale,
                       shift, a.smean, a.sinv, a.eps);
    return;
  }
  int rb;
  const float* part = bn_fwd_stats<T, VEC>(a, rb);
  if (apply_too)
    hipLaunchKernelGGL(bn_finalize_apply_kernel<T>, dim3(c), dim3(256), 0, a.st, part, rb, c, a.rows, a.gamma, a.beta, a.rmean,
                       a.rvar, a.smean, a.sinv, scale, shift, a.momentum, a.eps, a.nbt, (const T*)a.x, (const T*)a.res, (T*)a.y,
                       a.ldy, a.act);
  else
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(c), dim3(256), 0, a.st, part, rb, c, a.rows, a.gamma, a.beta, a.rmean, a.rvar,
                       a.smean, a.sinv, scale, shift, a.momentum, a.eps, a.nbt);
}
template <typename T, int VEC>
static void bn_fwd_launch(const BnArgs& a) {
  const bool tiny = a.training && a.rows <= kBnTinyRows;  // finalize + apply in one launch
  bn_fwd_coefs<T, VEC>(a, tiny);
  if (tiny) return;
  with_act(a.act, [&](auto av) {
    hipLaunchKernelGGL((bn_apply_kernel<T, VEC, decltype(av)::value>), bn_grid<VEC>(bn_apply_rb<VEC>(a.rows, a.c), a.c), dim3(256),
                       0, a.st, (const T*)a.x, (const T*)a.res, (T*)a.y, a.w.coef, a.w.coef + a.c, a.rows, a.c, a.act, a.ldy);
  });
}
// The forward's operands, as rtsds_bn_fwd_ld and rtsds_bn_relu_maxpool_fwd take them
static int bn_fwd_args(BnArgs& a, const float* gamma, const float* beta, float* running_mean, float* running_var,
                       long long* num_batches_tracked, float* save_mean, float* save_invstd, float momentum, float eps,
                       int training, const float* stats_part, int stats_nrb) {
  if (!training && (!running_mean || !running_var)) return RTSDS_ERR_UNSUPPORTED;
  if (training && (!save_mean || !save_invstd)) return RTSDS_ERR_UNSUPPORTED;
  a.affine(gamma, beta, save_mean, save_invstd);
  a.rmean = running_mean, a.rvar = running_var, a.nbt = training ? num_batches_tracked : nullptr;
  a.momentum = momentum, a.eps = eps, a.training = training;
  a.pre = stats_part, a.pre_nrb = stats_nrb;
  return RTSDS_OK;
}

extern "C" int rtsds_bn_fwd_ld(const void* x, const void* res, void* y, long ldy, long rows, int c, const float* gamma,
                               const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                               float* save_mean, float* save_invstd, float momentum, float eps, int training, int act,
                               const float* stats_part, int stats_nrb, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (rows <= 0 || c <= 0 || ldy < c) return RTSDS_ERR_SHAPE;
  if (ldy != c && !(dtype == RTSDS_BF16 && c % 8 == 0 && ldy % 8 == 0)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  BnArgs a(rows, c, ws, stream);
  if (int rc = bn_fwd_args(a, gamma, beta, running_mean, running_var, num_batches_tracked, save_mean, save_invstd, momentum, eps,
                           training, stats_part, stats_nrb))
    return rc;
  if (c > 65535 * 256) return RTSDS_ERR_UNSUPPORTED;
  a.x = x, a.res = res, a.y = y, a.ldy = ldy, a.act = act;
  if (int rc = bn_dispatch(dtype, c, [&](auto k) { bn_fwd_launch<typename decltype(k)::T, decltype(k)::VEC>(a); })) return rc;
  RET_LAUNCH();
}

extern "C" int rtsds_bn_fwd(const void* x, const void* res, void* y, long rows, int c, const float* gamma, const float* beta,
                            float* running_mean, float* running_var, long long* num_batches_tracked, float* save_mean,
                            float* save_invstd, float momentum,
                            float eps, int training, int act, const float* stats_part, int stats_nrb, int dtype, void* ws,
                            size_t ws_bytes, void* stream) {
  return rtsds_bn_fwd_ld(x, res, y, c, rows, c, gamma, beta, running_mean, running_var, num_batches_tracked, save_mean,
                         save_invstd, momentum, eps, training, act, stats_part, stats_nrb, dtype, ws, ws_bytes, stream);
}

template <typename T, int VEC, class GS>
static void bn_bwd_launch(const GS& gs, const BnArgs& a) {
  const T *x = (const T*)a.x, *y = (const T*)a.ykept;
  T *dx = (T*)a.dx, *dres = (T*)a.dres;
  const long rows = a.rows;
  const int c = a.c, act = a.act;
  // statistics already produced by the consumer conv's data-gradient epilogue, or our own pass's
  const int rb = a.pre ? a.pre_nrb : bn_bwd_rb<VEC>(rows, c);
  // residual BatchNorm + ReLU with both gradients wanted: the statistics pass stores
  // g = dy * relu'(y) as dres, and the apply pass reads g and x (not dy, y) -- one full read
  // less; g is exactly dy or 0, so the arithmetic is unchanged
  const bool g_out = !a.pre && y && act == RTSDS_ACT_RELU && dres && dx && GS::kDirect;
  // (coef_only: the one-launch form keeps its coefficients in LDS; the separate passes give the
  // same dgamma / dbeta bit for bit)
  if (!a.pre && rb == 1 && GS::kDirect && !g_out && !a.coef_only) {  // one row block: the three passes in one launch
    with_bool(y && act, [&](auto hy) {
      with_act(act, [&](auto av) {
        hipLaunchKernelGGL((bn_bwd_tiny_kernel<T, VEC, decltype(hy)::value, GS, decltype(av)::value>), bn_grid<VEC>(1, c), dim3(256),
                           0, a.st, gs, x, y, a.gamma, a.beta, a.smean, a.sinv, a.dgamma, a.dbeta, dx, dres, rows, c, act,
                           a.training, a.accumulate);
      });
    });
    return;
  }
  if (a.pre)  // channel-major [c][tile][2] partials of the data-gradient epilogue
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(c), dim3(256), 0, a.st, a.pre, rb, c, rows, a.gamma, a.beta, a.smean, a.sinv,
                       a.dgamma, a.dbeta, a.w.coef, a.training, a.accumulate);
  else {
    with_bool(y && act, [&](auto hy) {
      with_act(act, [&](auto av) {
        hipLaunchKernelGGL((bn_bwd_stats_kernel<T, VEC, decltype(hy)::value, GS, decltype(av)::value>), bn_grid<VEC>(rb, c), dim3(256),
                           0, a.st, gs, x, y, a.gamma, a.beta, a.smean, a.sinv, a.w.part, rows, c, act,
                           g_out ? dres : (T*)nullptr);
      });
    });
    hipLaunchKernelGGL(bn_bwd_finalize_rb_kernel, dim3(rt_cdiv(c, 16)), dim3(256), 0, a.st, a.w.part, rb, c, rows, a.gamma, a.beta,
                       a.smean, a.sinv, a.dgamma, a.dbeta, a.w.coef, a.training, a.accumulate);
  }
  const dim3 grid = bn_grid<VEC>(bn_apply_rb<VEC>(rows, c), c);
  if (g_out) {
    const GradDirect<T> gg{dres, c};
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, VEC, GradDirect<T>, RTSDS_ACT_NONE>), grid, dim3(256), 0, a.st, gg, x,
                       (const T*)nullptr, dx, (T*)nullptr, a.w.coef, rows, c, 0);
  } else if (dx || dres) {
    with_act(act, [&](auto av) {
      hipLaunchKernelGGL((bn_bwd_apply_kernel<T, VEC, GS, decltype(av)::value>), grid, dim3(256), 0, a.st, gs, x, y, dx, dres,
                         a.w.coef, rows, c, act);
    });
  }
}
template <typename T, int VEC>
static void bn_bwd_launch(const BnArgs& a) {
  const GradDirect<T> gs{(const T*)a.dy, (int)(a.ldy ? a.ldy : a.c)};
  bn_bwd_launch<T, VEC, GradDirect<T>>(gs, a);
}
// The backward's operands, as its three entry points take them
static void bn_bwd_args(BnArgs& a, const void* x, void* dx, float* dgamma, float* dbeta, const float* gamma, const float* beta,
                        const float* save_mean, const float* save_invstd, int training, int act, int accumulate) {
  a.affine(gamma, beta, save_mean, save_invstd);
  a.x = x, a.dx = dx, a.dgamma = dgamma, a.dbeta = dbeta;
  a.training = training, a.act = act, a.accumulate = accumulate;
}

extern "C" int rtsds_bn_bwd_part(const void* dy, const void* x, void* dx, float* dgamma, float* dbeta, long rows, int c,
                                 const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                                 int training, int act, int accumulate_params, const float* part, int nrb, int dtype, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (rows <= 0 || c <= 0 || nrb <= 0 || !part) return RTSDS_ERR_SHAPE;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  if (dtype != RTSDS_BF16 || c % 8 != 0) return RTSDS_ERR_UNSUPPORTED;
  if (!(act == RTSDS_ACT_NONE || act == RTSDS_ACT_RELU || act == RTSDS_ACT_LEAKY)) return RTSDS_ERR_UNSUPPORTED;
  BnArgs a(rows, c, ws, stream);
  bn_bwd_args(a, x, dx, dgamma, dbeta, gamma, beta, save_mean, save_invstd, training, act, accumulate_params);
  a.dy = dy, a.pre = part, a.pre_nrb = nrb;
  bn_bwd_launch<bf16, 8>(a);
  RET_LAUNCH();
}

extern "C" int rtsds_bn_bwd_ld(const void* dy, long ldy, const void* x, const void* y, void* dx, void* dres, float* dgamma,
                               float* dbeta, long rows, int c, const float* gamma, const float* beta, const float* save_mean,
                               const float* save_invstd, int training, int act, int accumulate_params, int dtype, void* ws,
                               size_t ws_bytes, void* stream) {
  if (rows <= 0 || c <= 0 || ldy < c || ldy > (1L << 30)) return RTSDS_ERR_SHAPE;
  if (ldy != c && !(dtype == RTSDS_BF16 && c % 8 == 0 && ldy % 8 == 0)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  if (!y && !(act == RTSDS_ACT_NONE || act == RTSDS_ACT_RELU || act == RTSDS_ACT_LEAKY)) return RTSDS_ERR_UNSUPPORTED;
  if (!y && act && dres) return RTSDS_ERR_UNSUPPORTED;  // residual: the mask needs y
  BnArgs a(rows, c, ws, stream);
  bn_bwd_args(a, x, dx, dgamma, dbeta, gamma, beta, save_mean, save_invstd, training, act, accumulate_params);
  a.dy = dy, a.ldy = ldy, a.ykept = y, a.dres = dres;
  if (int rc = bn_dispatch(dtype, c, [&](auto k) { bn_bwd_launch<typename decltype(k)::T, decltype(k)::VEC>(a); })) return rc;
  RET_LAUNCH();
}
// Statistics + finalize only: dgamma / dbeta as rtsds_bn_bwd, and the apply pass's coefficient rows
// [A | B | C | mean | scale | shift] x c into the caller's coef instead of the workspace -- for a
// consumer that applies dx = A*g + B*(x - mean) + C itself (rtsds_imgconv_bn_wgrad).
extern "C" int rtsds_bn_bwd_coef(const void* dy, const void* x, float* dgamma, float* dbeta, float* coef, long rows, int c,
                                 const float* gamma, const float* beta, const float* save_mean, const float* save_invstd,
                                 int training, int act, int accumulate_params, int dtype, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (rows <= 0 || c <= 0 || !coef || ((size_t)coef & 15)) return RTSDS_ERR_SHAPE;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  if (!(act == RTSDS_ACT_NONE || act == RTSDS_ACT_RELU || act == RTSDS_ACT_LEAKY)) return RTSDS_ERR_UNSUPPORTED;
  BnArgs a(rows, c, ws, stream);
  bn_bwd_args(a, x, nullptr, dgamma, dbeta, gamma, beta, save_mean, save_invstd, training, act, accumulate_params);
  a.dy = dy, a.w.coef = coef, a.coef_only = true;
  if (int rc = bn_dispatch(dtype, c, [&](auto k) { bn_bwd_launch<typename decltype(k)::T, decltype(k)::VEC>(a); })) return rc;
  RET_LAUNCH();
}
extern "C" int rtsds_bn_bwd(const void* dy, const void* x, const void* y, void* dx, void* dres, float* dgamma, float* dbeta,
                            long rows, int c, const float* gamma, const float* beta, const float* save_mean,
                            const float* save_invstd, int training, int act, int accumulate_params, int dtype, void* ws,
                            size_t ws_bytes, void* stream) {
  return rtsds_bn_bwd_ld(dy, c, x, y, dx, dres, dgamma, dbeta, rows, c, gamma, beta, save_mean, save_invstd, training, act,
                         accumulate_params, dtype, ws, ws_bytes, stream);
}

// ---- Training-mode residual BatchNorm + ReLU that keeps mask bits instead of y, and the pair of a
// residual block's last BatchNorm (A) with its downsample BatchNorm (B) on tensors of one shape.
// Every launch below computes what the separate calls above compute, bit for bit.
static bool bn_bits_ok(long rows, int c, int dtype) {
  return rows > 0 && c > 0 && c % 8 == 0 && c <= 65535 * 256 && (dtype == RTSDS_BF16 || dtype == RTSDS_F32);
}
extern "C" size_t rtsds_bn_bits_bytes(long rows, int c, int dtype) {
  if (!bn_bits_ok(rows, c, dtype)) return 0;
  return (size_t)rows * (c / (dtype == RTSDS_BF16 ? 8 : 4));
}
extern "C" size_t rtsds_bn_pair_workspace(long rows, int c) { return 2 * rtsds_bn_workspace(rows, c); }
// f(BnKind<T, VEC>) with VEC the 16-byte vector of the storage type (c % 8 == 0: always whole)
template <typename F>
static int bn_bits_dispatch(int dtype, F f) {
  if (dtype == RTSDS_BF16) f(BnKind<bf16, 8>());
  else if (dtype == RTSDS_F32) f(BnKind<float, 4>());
  else return RTSDS_ERR_UNSUPPORTED;
  return RTSDS_OK;
}

static int bn_params_fwd(BnArgs& a, const rtsds_bn_params* p) {
  return bn_fwd_args(a, p->gamma, p->beta, p->running_mean, p->running_var, p->num_batches_tracked, p->save_mean, p->save_invstd,
                     p->momentum, p->eps, 1, p->stats_part, p->stats_nrb);
}
template <typename T, int VEC>
static void bn_bits_fwd_launch(const BnArgs& a, const BnArgs* b, uint8_t* bits) {
  const int c = a.c;
  const dim3 grid = bn_grid<VEC>(bn_apply_rb<VEC>(a.rows, c), c);
  if (!b) {
    bn_fwd_coefs<T, VEC>(a);
    hipLaunchKernelGGL((bn_apply_bits_kernel<T, VEC, false>), grid, dim3(256), 0, a.st, (const T*)a.x, (const T*)a.res, (T*)a.y, bits,
                       a.w.coef, a.w.coef + c, (const float*)nullptr, (const float*)nullptr, a.rows, c);
    return;
  }
  BnFin f[2];
  const BnArgs* ab[2] = {&a, b};
  for (int i = 0; i < 2; ++i) {
    const BnArgs& q = *ab[i];
    int rb;
    const float* part = bn_fwd_stats<T, VEC>(q, rb);
    f[i] = BnFin{part, rb, q.gamma, q.beta, q.rmean, q.rvar, q.smean, q.sinv, q.w.coef, q.w.coef + c, q.momentum, q.eps, q.nbt};
  }
  hipLaunchKernelGGL(bn_finalize_pair_kernel, dim3(c, 2), dim3(256), 0, a.st, f[0], f[1], c, a.rows);
  hipLaunchKernelGGL((bn_apply_bits_kernel<T, VEC, true>), grid, dim3(256), 0, a.st, (const T*)a.x, (const T*)b->x, (T*)a.y, bits,
                     a.w.coef, a.w.coef + c, b->w.coef, b->w.coef + c, a.rows, c);
}
template <typename T, int VEC>
static void bn_bits_bwd_launch(const BnArgs& a, const BnArgs* b, const uint8_t* bits) {
  const T* x = (const T*)a.x;
  const long rows = a.rows;
  const int c = a.c;
  const GradDirect<T> gs{(const T*)a.dy, (int)(a.ldy ? a.ldy : c)};
  const int rb = bn_bwd_rb<VEC>(rows, c);
  const dim3 sgrid = bn_grid<VEC>(rb, c), agrid = bn_grid<VEC>(bn_apply_rb<VEC>(rows, c), c);
  if (!b) {
    // as bn_bwd_launch's g_out route: the statistics pass stores g as dres, the apply reads g and x
    hipLaunchKernelGGL((bn_bwd_stats_bits_kernel<T, VEC, GradDirect<T>, false>), sgrid, dim3(256), 0, a.st, gs, x, bits, a.gamma,
                       a.beta, a.smean, a.sinv, a.w.part, rows, c, (T*)a.dres, (const T*)nullptr, (const float*)nullptr,
                       (float*)nullptr);
    hipLaunchKernelGGL(bn_bwd_finalize_rb_kernel, dim3(rt_cdiv(c, 16)), dim3(256), 0, a.st, a.w.part, rb, c, rows, a.gamma, a.beta,
                       a.smean, a.sinv, a.dgamma, a.dbeta, a.w.coef, 1, a.accumulate);
    const GradDirect<T> gg{(const T*)a.dres, c};
    hipLaunchKernelGGL((bn_bwd_apply_kernel<T, VEC, GradDirect<T>, RTSDS_ACT_NONE>), agrid, dim3(256), 0, a.st, gg, x,
                       (const T*)nullptr, (T*)a.dx, (T*)nullptr, a.w.coef, rows, c, 0);
    return;
  }
  hipLaunchKernelGGL((bn_bwd_stats_bits_kernel<T, VEC, GradDirect<T>, true>), sgrid, dim3(256), 0, a.st, gs, x, bits, a.gamma, a.beta,
                     a.smean, a.sinv, a.w.part, rows, c, (T*)nullptr, (const T*)b->x, b->smean, b->w.part);
  const BnBwdFin fa{a.w.part, a.gamma, a.beta, a.smean, a.sinv, a.dgamma, a.dbeta, a.w.coef, a.accumulate};
  const BnBwdFin fb{b->w.part, b->gamma, b->beta, b->smean, b->sinv, b->dgamma, b->dbeta, b->w.coef, b->accumulate};
  hipLaunchKernelGGL(bn_bwd_finalize_pair_kernel, dim3(rt_cdiv(c, 16), 2), dim3(256), 0, a.st, fa, fb, rb, c, rows);
  hipLaunchKernelGGL((bn_bwd_apply_pair_kernel<T, VEC, GradDirect<T>>), agrid, dim3(256), 0, a.st, gs, bits, x, (const T*)b->x,
                     (T*)a.dx, (T*)b->dx, a.w.coef, b->w.coef, rows, c);
}

extern "C" int rtsds_bn_fwd_bits(const void* x, const void* res, void* y, uint8_t* bits, long rows, int c, const float* gamma,
                                 const float* beta, float* running_mean, float* running_var, long long* num_batches_tracked,
                                 float* save_mean, float* save_invstd, float momentum, float eps, const float* stats_part,
                                 int stats_nrb, int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (rows <= 0 || c <= 0 || !x || !res || !y || !bits) return RTSDS_ERR_SHAPE;
  if (!bn_bits_ok(rows, c, dtype)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  BnArgs a(rows, c, ws, stream);
  if (int rc = bn_fwd_args(a, gamma, beta, running_mean, running_var, num_batches_tracked, save_mean, save_invstd, momentum, eps, 1,
                           stats_part, stats_nrb))
    return rc;
  a.x = x, a.res = res, a.y = y, a.ldy = c, a.act = RTSDS_ACT_RELU;
  if (int rc = bn_bits_dispatch(dtype, [&](auto k) { bn_bits_fwd_launch<typename decltype(k)::T, decltype(k)::VEC>(a, nullptr, bits); }))
    return rc;
  RET_LAUNCH();
}
extern "C" int rtsds_bn_bwd_bits(const void* dy, long ldy, const void* x, const uint8_t* bits, void* dx, void* dres, float* dgamma,
                                 float* dbeta, long rows, int c, const float* gamma, const float* beta, const float* save_mean,
                                 const float* save_invstd, int accumulate_params, int dtype, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (rows <= 0 || c <= 0 || ldy < c || ldy > (1L << 30) || !dy || !x || !bits || !dx || !dres) return RTSDS_ERR_SHAPE;
  if (!bn_bits_ok(rows, c, dtype)) return RTSDS_ERR_UNSUPPORTED;
  if (ldy != c && !(dtype == RTSDS_BF16 && ldy % 8 == 0)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  BnArgs a(rows, c, ws, stream);
  bn_bwd_args(a, x, dx, dgamma, dbeta, gamma, beta, save_mean, save_invstd, 1, RTSDS_ACT_RELU, accumulate_params);
  a.dy = dy, a.ldy = ldy, a.dres = dres;
  if (int rc = bn_bits_dispatch(dtype, [&](auto k) { bn_bits_bwd_launch<typename decltype(k)::T, decltype(k)::VEC>(a, nullptr, bits); }))
    return rc;
  RET_LAUNCH();
}
extern "C" int rtsds_bn_pair_fwd(const void* xa, const void* xb, void* y, uint8_t* bits, long rows, int c,
                                 const rtsds_bn_params* pa, const rtsds_bn_params* pb, int dtype, void* ws, size_t ws_bytes,
                                 void* stream) {
  if (rows <= 0 || c <= 0 || !xa || !xb || !y || !bits || !pa || !pb) return RTSDS_ERR_SHAPE;
  if (!bn_bits_ok(rows, c, dtype)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_pair_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  BnArgs a(rows, c, ws, stream), b(rows, c, (char*)ws + rtsds_bn_workspace(rows, c), stream);
  if (int rc = bn_params_fwd(a, pa)) return rc;
  if (int rc = bn_params_fwd(b, pb)) return rc;
  a.x = xa, a.y = y, a.ldy = c, a.act = RTSDS_ACT_RELU, b.x = xb;
  if (int rc = bn_bits_dispatch(dtype, [&](auto k) { bn_bits_fwd_launch<typename decltype(k)::T, decltype(k)::VEC>(a, &b, bits); }))
    return rc;
  RET_LAUNCH();
}
extern "C" int rtsds_bn_pair_bwd(const void* dy, long ldy, const void* xa, const void* xb, const uint8_t* bits, void* dxa, void* dxb,
                                 long rows, int c, const rtsds_bn_params* pa, const rtsds_bn_params* pb, int dtype, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (rows <= 0 || c <= 0 || ldy < c || ldy > (1L << 30) || !dy || !xa || !xb || !bits || !dxa || !dxb || !pa || !pb)
    return RTSDS_ERR_SHAPE;
  if (!bn_bits_ok(rows, c, dtype)) return RTSDS_ERR_UNSUPPORTED;
  if (ldy != c && !(dtype == RTSDS_BF16 && ldy % 8 == 0)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_pair_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  BnArgs a(rows, c, ws, stream), b(rows, c, (char*)ws + rtsds_bn_workspace(rows, c), stream);
  bn_bwd_args(a, xa, dxa, pa->dgamma, pa->dbeta, pa->gamma, pa->beta, pa->save_mean, pa->save_invstd, 1, RTSDS_ACT_RELU,
              pa->accumulate);
  bn_bwd_args(b, xb, dxb, pb->dgamma, pb->dbeta, pb->gamma, pb->beta, pb->save_mean, pb->save_invstd, 1, RTSDS_ACT_NONE,
              pb->accumulate);
  a.dy = dy, a.ldy = ldy;
  if (int rc = bn_bits_dispatch(dtype, [&](auto k) { bn_bits_bwd_launch<typename decltype(k)::T, decltype(k)::VEC>(a, &b, bits); }))
    return rc;
  RET_LAUNCH();
}

// Training-mode BatchNorm + activation of an [n][hw][c] feature whose global average pool is wanted
// too: statistics / finalize as rtsds_bn_fwd, then one pass that applies and leaves the pool's
// stage-1 partials (gap_part: rtsds_gap_workspace(n, hw, c) bytes, [n][chan_slices][c]).
extern "C" int rtsds_bn_fwd_gap(const void* x, void* y, float* gap_part, int n, long hw, int c, const float* gamma, const float* beta,
                                float* running_mean, float* running_var, long long* num_batches_tracked, float* save_mean,
                                float* save_invstd, float momentum, float eps, int act, const float* stats_part, int stats_nrb,
                                int dtype, void* ws, size_t ws_bytes, void* stream) {
  if (n <= 0 || n > 65535 || hw <= 0 || c <= 0 || !x || !y || !gap_part) return RTSDS_ERR_SHAPE;
  const long rows = (long)n * hw;
  // the pool's scalar route only (c off the vector multiples), one channel chunk
  if (c > 256 || c % (dtype == RTSDS_BF16 ? 8 : 4) == 0) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  BnArgs a(rows, c, ws, stream);
  if (int rc = bn_fwd_args(a, gamma, beta, running_mean, running_var, num_batches_tracked, save_mean, save_invstd, momentum, eps,
                           1, stats_part, stats_nrb))
    return rc;
  a.x = x, a.y = y, a.ldy = c, a.act = act;
  DISPATCH_T(dtype, {
    bn_fwd_coefs<T, 1>(a);
    hipLaunchKernelGGL(bn_apply_gap_kernel<T>, dim3(chan_slices(n, hw), n, 1), dim3(256), 0, a.st, (const T*)x, (T*)y, a.w.coef,
                       a.w.coef + c, gap_part, hw, c, act);
  });
  RET_LAUNCH();
}
// rtsds_bn_bwd for the FeatureFusionModule's ConvBlock with the incoming gradient formed per element
// from its two readers' (GradScalePool): dr [n][hw][c] the channel scale's output gradient,
// att / dpooled [n][c].  No activation output kept (the mask is recomputed from x).
extern "C" int rtsds_bn_bwd_ffm(const void* dr, const void* att, const void* dpooled, int n, long hw, const void* x, void* dx,
                                float* dgamma, float* dbeta, int c, const float* gamma, const float* beta, const float* save_mean,
                                const float* save_invstd, int training, int act, int accumulate_params, int dtype, void* ws,
                                size_t ws_bytes, void* stream) {
  if (n <= 0 || hw <= 0 || c <= 0 || !dr || !att || !dpooled || !x) return RTSDS_ERR_SHAPE;
  const long rows = (long)n * hw;
  if (c % (dtype == RTSDS_BF16 ? 8 : 4) == 0) return RTSDS_ERR_UNSUPPORTED;  // one channel per thread
  if (!(act == RTSDS_ACT_NONE || act == RTSDS_ACT_RELU || act == RTSDS_ACT_LEAKY)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  BnArgs a(rows, c, ws, stream);
  bn_bwd_args(a, x, dx, dgamma, dbeta, gamma, beta, save_mean, save_invstd, training, act, accumulate_params);
  DISPATCH_T(dtype, {
    const GradScalePool<T> gs{(const T*)dr, (const T*)att, (const T*)dpooled, c, hw, 1.f / (float)hw};
    bn_bwd_launch<T, 1, GradScalePool<T>>(gs, a);
  });
  RET_LAUNCH();
}

// ---- BatchNorm + ReLU + MaxPool2d(3, 2, p) (the ResNet stem: bn1 -> relu -> maxpool,
// build_contextpath.py:15-18 / torchvision resnet.py; deeplabv2.py:106-110 with ceil mode).
// Forward: the pool reads the conv output and applies the BatchNorm scale / shift + ReLU to
// each window value (rounded to the storage dtype, exactly the value the separate bn_apply
// would have stored), so the full-resolution activation is never written; the window argmax
// bytes are stored for the backward, which gathers the pooled gradient inside the BatchNorm
// backward passes (GradPool) -- the full-resolution gradient is never written either.
template <typename T>
__global__ void __launch_bounds__(256) bn_relu_pool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ scale,
                                                              const float* __restrict__ shift, T* __restrict__ y,
                                                              uint8_t* __restrict__ idx, int h, int w, int c, int ho, int wo, int p,
                                                              long total, FastDiv f_cv, FastDiv f_wo, FastDiv f_ho) {
  typedef typename VecT<T>::v16 V16;
  constexpr int V = VecT<T>::N;
  const int cv = c / V;
  const int nwg = gridDim.x, bx = blockIdx.x, xcd = bx & 7, qq = nwg >> 3, rr = nwg & 7;  // XCD-contiguous blocks
  const long lb = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bx >> 3);
  for (long i = lb * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const uint32_t ii = (uint32_t)i, q0 = fdiv(ii, f_cv), q1 = fdiv(q0, f_wo), img = fdiv(q1, f_ho);
    const int ch = (int)(ii - q0 * cv) * V;
    const int ow = (int)(q0 - q1 * wo), oh = (int)(q1 - img * ho);
    const int h0 = oh * 2 - p, w0 = ow * 2 - p;
    V16 v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hh = min(max(h0 + t / 3, 0), h - 1), ww = min(max(w0 + t % 3, 0), w - 1);
      v[t] = *(const V16*)(x + (((long)img * h + hh) * w + ww) * c + ch);
    }
    float sc[V], sh[V];
    load_coef<V>(scale, ch, c, sc);
    load_coef<V>(shift, ch, c, sh);
    float best[V];
    int bi[V];
#pragma unroll
    for (int j = 0; j < V; ++j) { best[j] = -INFINITY; bi[j] = -1; }
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int hh = h0 + t / 3, ww = w0 + t % 3;
      if ((unsigned)hh >= (unsigned)h || (unsigned)ww >= (unsigned)w) continue;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float f = to_f(from_f<T>(fmaxf(fmaf(to_f(v[t][j]), sc[j], sh[j]), 0.f)));
        if (bi[j] < 0 || f > best[j] || (f != f && best[j] == best[j])) { best[j] = f; bi[j] = t; }
      }
    }
    V16 o;
    const long oi = (((long)img * ho + oh) * wo + ow) * c + ch;
    unsigned long long ib = 0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      o[j] = from_f<T>(best[j]);
      ib |= (unsigned long long)(bi[j] < 0 ? 0 : bi[j]) << (8 * j);
    }
    *(V16*)(y + oi) = o;
    *(unsigned long long*)(idx + oi) = ib;
  }
}
static bool bn_pool_ok(int n, int h, int w, int c, int ho, int wo, int p, int dtype) {
  return dtype == RTSDS_BF16 && c % 8 == 0 && n > 0 && ho > 0 && wo > 0 && (p == 0 || p == 1) &&
         (long)n * h * w * c < (1L << 31) && (long)n * ho * wo * c < (1L << 31);
}
extern "C" int rtsds_bn_relu_maxpool_fwd(const void* x, void* y, uint8_t* idx, int n, int h, int w, int c, int ho, int wo, int p,
                                         const float* gamma, const float* beta, float* running_mean, float* running_var,
                                         long long* num_batches_tracked, float* save_mean, float* save_invstd, float momentum,
                                         float eps, int training, const float* stats_part, int stats_nrb, int dtype, void* ws,
                                         size_t ws_bytes, void* stream) {
  const long rows = (long)n * h * w;
  if (!bn_pool_ok(n, h, w, c, ho, wo, p, dtype)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  BnArgs a(rows, c, ws, stream);
  if (int rc = bn_fwd_args(a, gamma, beta, running_mean, running_var, num_batches_tracked, save_mean, save_invstd, momentum, eps,
                           training, stats_part, stats_nrb))
    return rc;
  a.x = x;
  bn_fwd_coefs<bf16, 8>(a);
  hipStream_t st = a.st;
  const float *scale = a.w.coef, *shift = a.w.coef + c;
  const long total = (long)n * ho * wo * (c / 8);
  const int blocks = (int)std::max<long>(1, std::min<long>((total + 255) / 256, 1L << 20));
  hipLaunchKernelGGL(bn_relu_pool_fwd_kernel<bf16>, dim3(blocks), dim3(256), 0, st, (const bf16*)x, scale, shift, (bf16*)y, idx, h, w, c, ho, wo, p, total, fastdiv_make(c / 8), fastdiv_make(wo),
                     fastdiv_make(ho));
  RET_LAUNCH();
}
extern "C" int rtsds_bn_relu_maxpool_bwd(const void* dy_pool, const uint8_t* idx, const void* x, void* dx, float* dgamma,
                                         float* dbeta, int n, int h, int w, int c, int ho, int wo, int p, const float* gamma,
                                         const float* beta, const float* save_mean, const float* save_invstd, int training,
                                         int accumulate_params, int dtype, void* ws, size_t ws_bytes, void* stream) {
  const long rows = (long)n * h * w;
  if (!bn_pool_ok(n, h, w, c, ho, wo, p, dtype)) return RTSDS_ERR_UNSUPPORTED;
  if (ws_bytes < rtsds_bn_workspace(rows, c)) return RTSDS_ERR_WORKSPACE;
  const GradPool<bf16> gs{(const bf16*)dy_pool, idx, c, h, w, ho, wo, p, fastdiv_make(w), fastdiv_make(h)};
  BnArgs a(rows, c, ws, stream);
  bn_bwd_args(a, x, dx, dgamma, dbeta, gamma, beta, save_mean, save_invstd, training, RTSDS_ACT_RELU, accumulate_params);
  bn_bwd_launch<bf16, 8, GradPool<bf16>>(gs, a);
  RET_LAUNCH();
}

// Eval-mode BatchNorm folded into the producing conv (rtsds_conv2d_fwd_bn):
// scale = gamma / sqrt(running_var + eps), shift = beta + (bias - running_mean) * scale.
__global__ void bn_fold_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ rm, const float* __restrict__ rv,
                               const float* __restrict__ bias, float eps, int c, float* __restrict__ scale,
                               float* __restrict__ shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= c) return;
  const float s = (gamma ? gamma[i] : 1.f) / sqrtf(rv[i] + eps);
  scale[i] = s;
  shift[i] = fmaf((bias ? bias[i] : 0.f) - rm[i], s, beta ? beta[i] : 0.f);
}

extern "C" int rtsds_bn_fold(const float* gamma, const float* beta, const float* running_mean,
                             const float* running_var, const float* conv_bias, float eps, int c, float* scale,
                             float* shift, void* stream) {
  if (c <= 0) return RTSDS_ERR_SHAPE;
  if (!running_mean || !running_var || !scale || !shift) return RTSDS_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(bn_fold_kernel, dim3(rt_cdiv(c, 256)), dim3(256), 0, (hipStream_t)stream, gamma, beta, running_mean,
                     running_var, conv_bias, eps, c, scale, shift);
  RET_LAUNCH();
}
