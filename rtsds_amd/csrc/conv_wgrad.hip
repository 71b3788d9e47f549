// Convolution weight (and bias) gradient, host side (C ABI): the pooled, narrow-pointwise and
// halo (hconv.hip nwgrad) routes or the split-K implicit GEMM (conv_gemm_kernel.h, instantiated
// in conv_gemm_wgrad.hip), the workspace plan, and the helper kernels: split-K reductions, bias
// column sums, the narrow pointwise gradient, the superpixel dW unpack.
#include "conv_host.h"
#include "split_reduce_dev.h"

// dw[co][tap][ci] = sum_s part[s][co][tap][ci_p]   (split-K reduce + channel unpad).
// V consecutive input channels per thread (16-byte slab reads when c % 4 == 0), splits
// summed in a fixed order -- deterministic, no atomics.
// Block = 64 outputs x 4 split groups (wave g sums splits g, g + 4, ... in order; the four
// group sums are then added in group order): the many-split reductions of small weight
// tensors (ResNet layer1: ~100 splits) get 4x the parallelism of one thread per output.
template <int V>
__global__ void __launch_bounds__(256) split_reduce_kernel(const float* __restrict__ part, float* __restrict__ out, int nv,
                                                            int cv, FastDiv fcv, int cp, long slab, int splits, int accumulate) {
  __shared__ float red[4][64][V];
  const int lane = threadIdx.x & 63, sg = threadIdx.x >> 6;
  for (int i0 = blockIdx.x * 64; i0 < nv; i0 += gridDim.x * 64) {
    const int i = i0 + lane;
    const bool ok = i < nv;
    const int rt = (int)fdiv((uint32_t)(ok ? i : 0), fcv);  // co * taps + tap
    const long src = (long)rt * cp + (long)((ok ? i : 0) - rt * cv) * V;
    float s[V];
#pragma unroll
    for (int e = 0; e < V; ++e) s[e] = 0.f;
    // splits sg, sg + 4, ... summed in order; 8 loads in flight per thread (clamped,
    // unconditional; past-the-end ones contribute nothing)
    for (int q = sg; ok && q < splits; q += 32) {
      float t[8][V];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const long off = (long)min(q + 4 * u, splits - 1) * slab + src;
        if constexpr (V == 4) {
          const f32x4 v = *(const f32x4*)(part + off);
#pragma unroll
          for (int e = 0; e < V; ++e) t[u][e] = v[e];
        } else {
          t[u][0] = part[off];
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (q + 4 * u < splits)
#pragma unroll
          for (int e = 0; e < V; ++e) s[e] += t[u][e];
    }
#pragma unroll
    for (int e = 0; e < V; ++e) red[sg][lane][e] = s[e];
    __syncthreads();
    if (sg == 0 && ok) {
      float* o = out + (long)i * V;
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float t = (red[0][lane][e] + red[1][lane][e]) + (red[2][lane][e] + red[3][lane][e]);
        o[e] = accumulate ? o[e] + t : t;
      }
    }
    __syncthreads();
  }
}

// dbias: two-stage deterministic column sum of dy[rows][c].  Stage 1: grid (RB, channel
// chunks); 256 threads laid out [row group][channel vector] (coalesced whole-row reads);
// block b sums rows b*rpi + rg (+= RB*rpi) -> part[b][c].  Stage 2 sums the RB partials.
template <typename T, int VEC>
__global__ void __launch_bounds__(256) colsum_part_kernel(const T* __restrict__ dy, float* __restrict__ part, long rows, int c) {
  __shared__ float red[256 * VEC];
  const int cbase = blockIdx.y * 256 * VEC;
  const int cl = min(c - cbase, 256 * VEC);
  const int tpr = (cl + VEC - 1) / VEC, rpi = 256 / tpr;
  const int tid = threadIdx.x, cv = tid % tpr, rg = tid / tpr;
  const int ch0 = cbase + cv * VEC;
  float acc[VEC];
#pragma unroll
  for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
  if (rg < rpi) {
    // 4 rows' loads in flight (clamped, unconditional), then the adds in row order
    const long step = (long)gridDim.x * rpi;
    for (long r = (long)blockIdx.x * rpi + rg; r < rows; r += 4 * step) {
      typename VecT<T>::v16 v[4];
      T sv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long rr = min(r + u * step, rows - 1);
        if (VEC > 1) v[u] = *(const typename VecT<T>::v16*)(dy + rr * c + ch0);
        else sv[u] = dy[rr * c + ch0];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (r + u * step < rows) {
          if (VEC > 1) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[j] += to_f(v[u][j]);
          } else {
            acc[0] += to_f(sv[u]);
          }
        }
    }
  }
#pragma unroll
  for (int j = 0; j < VEC; ++j) red[tid * VEC + j] = acc[j];
  __syncthreads();
  if (rg == 0) {
    for (int g = 1; g < rpi; ++g)
#pragma unroll
      for (int j = 0; j < VEC; ++j) acc[j] += red[(g * tpr + cv) * VEC + j];
#pragma unroll
    for (int j = 0; j < VEC; ++j)
      if (ch0 + j < c) part[(long)blockIdx.x * c + ch0 + j] = acc[j];
  }
}
// colsum_part_kernel<T, 1> (the same layout, loop and reduction: bit-identical partials) that
// also writes the gradient's channel-padded copy [rows][cp] the weight-gradient GEMM reads
// (pad_channels_kernel's job) -- one launch and one read of dY for both (c <= 256).
template <typename T>
__global__ void __launch_bounds__(256) pad_colsum_kernel(const T* __restrict__ dy, T* __restrict__ dyp, float* __restrict__ part,
                                                         long rows, int c, int cp) {
  __shared__ float red[256];
  const int tpr = c, rpi = 256 / tpr;
  const int tid = threadIdx.x, cv = tid % tpr, rg = tid / tpr;
  float acc = 0.f;
  if (rg < rpi) {
    const long step = (long)gridDim.x * rpi;
    for (long r = (long)blockIdx.x * rpi + rg; r < rows; r += 4 * step) {
      T sv[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) sv[u] = dy[min(r + u * step, rows - 1) * c + cv];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long rr = r + u * step;
        if (rr < rows) {
          acc += to_f(sv[u]);
          T* o = dyp + rr * cp;
          o[cv] = sv[u];
          for (int pc = c + cv; pc < cp; pc += tpr) o[pc] = from_f<T>(0.f);
        }
      }
    }
  }
  red[tid] = acc;
  __syncthreads();
  if (rg == 0) {
    for (int g = 1; g < rpi; ++g) acc += red[g * tpr + cv];
    part[(long)blockIdx.x * c + cv] = acc;
  }
}
__global__ void colsum_final_kernel(const float* __restrict__ part, float* __restrict__ out, int rb, int c, int accumulate) {
  const int cc = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int i0 = lane; i0 < rb; i0 += 64 * 8) {  // 8 partials in flight (clamped), added in order
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = part[(long)min(i0 + 64 * u, rb - 1) * c + cc];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 + 64 * u < rb) s += t[u];
  }
  s = wave_sum(s);
  if (lane == 0) out[cc] = accumulate ? out[cc] + s : s;
}
static const int kColsumRB = 1024;

// dW'[k][r][p][8] (fp32) -> dw[k][r][s][3] (+=).
__global__ void __launch_bounds__(256) sp_unpack_dw_kernel(const float* __restrict__ dwp, float* __restrict__ dw, int k, int kh,
                                                           int kw, int kwp, int accumulate) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= k * kh * kw * 3) return;
  const int ch = i % 3, t = i / 3;
  const int s = t % kw, kr = t / kw;
  const int p = (s + 1) >> 1, q = (s + 1) & 1;
  const float v = dwp[((long)kr * kwp + p) * 8 + q * 4 + ch];
  dw[i] = accumulate ? dw[i] + v : v;
}

// ---- narrow pointwise weight + bias gradient (1x1, stride 1, Cin and Cout <= 32: BiSeNet's final
// 19 -> 19 conv, build_bisenet.py:117).  As a GEMM it needed dY and x padded to 32 channels, a
// split-K launch, its reduce and the bias column sums' two launches -- six launches for 0.05 GFLOP.
// Here: pass 1, one workgroup per run of kPwnRows pixels stages 64-pixel tiles of dY and x in LDS
// and accumulates every (co, ci) product and the dY column sums -> part[block][k*c dW | k db];
// pass 2 (one wave per output) sums the blocks in a fixed order.
static constexpr int kPwnRows = 128;
static bool pwn_wgrad_ok(const rtsds_conv_desc* d) {
  // (k <= 28: 9 threads per output row in a 256-thread workgroup)
  return d->kh == 1 && d->kw == 1 && d->sh == 1 && d->sw == 1 && d->ph == 0 && d->pw == 0 && d->k <= 28 && d->c <= 32;
}
static int pwn_blocks(const rtsds_conv_desc* d) {
  return (int)std::min<long>(4096, ((long)d->n * d->h * d->w + kPwnRows - 1) / kPwnRows);
}
template <typename T>
__global__ void __launch_bounds__(256) pwn_wgrad_part_kernel(const T* __restrict__ dy, const T* __restrict__ x, float* __restrict__ part,
                                                             long P, int k, int c, int ldx, int per) {
  // thread t: output row co = t / 9, column group g = t % 9 -- dW[co][4g .. 4g + 3] for g < 8, the
  // bias sum (x's ones column 32) for g = 8; one dY read and one 16-B x read per pixel, 4 FMAs
  __shared__ float sdy[64][33];
  __shared__ __attribute__((aligned(16))) float sx[64][36];
  const long p0 = (long)blockIdx.x * per, p1 = min(P, p0 + per);
  const int co = threadIdx.x / 9, g = threadIdx.x - co * 9;
  const bool active = co < k && (g == 8 || 4 * g < c);
  const int coc = min(co, 31);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (long pb = p0; pb < p1; pb += 64) {
    const int np = (int)min(64L, p1 - pb);
    __syncthreads();
    // 64 x 32 elements of each tensor, 8 per thread: clamped unconditional loads, then the
    // zero fill past the pixels / channels selected
    float vd[8], vx[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = threadIdx.x + 256 * u, r = e >> 5, ch = e & 31;
      const long pr = pb + min(r, np - 1);
      vd[u] = to_f(dy[pr * k + min(ch, k - 1)]);
      vx[u] = to_f(x[pr * ldx + min(ch, c - 1)]);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = threadIdx.x + 256 * u, r = e >> 5, ch = e & 31;
      sdy[r][ch] = (r < np && ch < k) ? vd[u] : 0.f;
      sx[r][ch] = (r < np && ch < c) ? vx[u] : 0.f;
    }
    if (threadIdx.x < 64) *(f32x4*)&sx[threadIdx.x][32] = f32x4{threadIdx.x < np ? 1.f : 0.f, 0.f, 0.f, 0.f};
    __syncthreads();
    if (active) {
#pragma unroll 8
      for (int r = 0; r < 64; ++r) {
        const float d = sdy[r][coc];
        const f32x4 v = *(const f32x4*)&sx[r][4 * g];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = fmaf(d, v[j], acc[j]);
      }
    }
  }
  if (!active) return;
  const int no = k * c + k;
  float* out = part + (long)blockIdx.x * no;
  if (g == 8) {
    out[k * c + co] = acc[0];
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * g + j < c) out[co * c + 4 * g + j] = acc[j];
  }
}
// one wave per output: lane l sums the partials of blocks l, l + 64, ... (8 in flight, in
// order), then the wave's fixed shuffle tree
__global__ void __launch_bounds__(64) pwn_wgrad_final_kernel(const float* __restrict__ part, float* __restrict__ dw,
                                                             float* __restrict__ dbias, int nb, int k, int c, int accum) {
  const int no = k * c + k, o = blockIdx.x, lane = threadIdx.x;
  float s = 0.f;
  for (int b0 = lane; b0 < nb; b0 += 64 * 8) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) t[u] = part[(long)min(b0 + 64 * u, nb - 1) * no + o];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (b0 + 64 * u < nb) s += t[u];
  }
  s = wave_sum(s);
  if (lane != 0) return;
  if (o < k * c) dw[o] = accum ? dw[o] + s : s;
  else if (dbias) dbias[o - k * c] = accum ? dbias[o - k * c] + s : s;
}

// Batched split-K reductions (rtsds_split_reduce_many): block b belongs to the descriptor whose
// block range contains it; within it, split_reduce_kernel<4>'s arithmetic (4 split groups per
// 64 outputs, summed in split order) -- bit-identical to the per-wgrad launch.
static const int kReduceBatch = 16;
struct ReduceBatch {
  rtsds_split_reduce_desc d[kReduceBatch];
  int blk0[kReduceBatch];
  int n;
};
__global__ void __launch_bounds__(256) split_reduce_many_kernel(const ReduceBatch b) {
  __shared__ float red[4][64][4];
  int si = 0;
  for (int i = 1; i < b.n; ++i)
    if (b.blk0[i] <= (int)blockIdx.x) si = i;
  const rtsds_split_reduce_desc& q = b.d[si];
  const int lane = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int i = ((int)blockIdx.x - b.blk0[si]) * 64 + lane;
  float t[4];
  split_reduce_block(q, i, red, t);  // (split_reduce_dev.h: shared with the fused Adam step)
  if (sg == 0 && i < q.nv) {
    float* o = q.dw + (long)i * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = q.accumulate ? o[e] + t[e] : t[e];
  }
}
extern "C" int rtsds_split_reduce_many(int n, const rtsds_split_reduce_desc* descs, void* stream) {
  if (n < 0 || (n && !descs)) return RTSDS_ERR_SHAPE;
  for (int i0 = 0; i0 < n; i0 += kReduceBatch) {
    ReduceBatch b;
    b.n = 0;
    int blocks = 0;
    for (int i = i0; i < n && b.n < kReduceBatch; ++i) {
      if (descs[i].nv <= 0) continue;
      if (descs[i].cv <= 0 || descs[i].splits <= 0 || !descs[i].slab || !descs[i].dw) return RTSDS_ERR_SHAPE;
      b.d[b.n] = descs[i];
      b.blk0[b.n] = blocks;
      blocks += (descs[i].nv + 63) / 64;
      ++b.n;
    }
    if (b.n) hipLaunchKernelGGL(split_reduce_many_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b);
  }
  RET_LAUNCH();
}


// ---- host side ---------------------------------------------------------------------------
// One plan for the workspace query and the launch: the GEMM's view g of the conv (the superpixel
// geometry of the 3-channel stride-2 image convs, else the conv itself), its tile and split-K
// choice, and the workspace regions in this order: [split-K slabs][Cout-padded dY][Cin-padded x]
// [bias column-sum partials][superpixel image][dW' before the unpack].  The narrow pointwise
// route's partials lie alone at the base.
struct WgradPlan {
  rtsds_conv_desc g;
  bool sp, nw;
  int kp, cp, bm, bn, splits, tps;
  size_t slab_bytes, dyp_bytes, xp_bytes, colsum_bytes, x4_bytes, dws_bytes, pwn_bytes;
  size_t total() const {
    return std::max(slab_bytes + dyp_bytes + xp_bytes + colsum_bytes + x4_bytes + dws_bytes, pwn_bytes);
  }
};
// the halo-direct weight gradient of a narrow-output 3x3 conv (hconv.hip nwgrad): dY padded to 32
// channels, one slab per run of tiles, the same split reduce
static bool nw_path(const rtsds_conv_desc* d) { return pad_c(d->k, d->dtype) == 32 && nwgrad_ok(d); }
static constexpr auto kWgradWant = 512;
static WgradPlan wgrad_plan(const rtsds_conv_desc* d0) {
  WgradPlan w = {};
  w.sp = sp_path(d0);
  w.g = w.sp ? sp_desc(d0) : *d0;
  const rtsds_conv_desc* d = &w.g;
  const bool b16 = d->dtype == RTSDS_BF16;
  const size_t es = esize(d->dtype);
  w.kp = pad_c(d->k, d->dtype);
  w.cp = pad_c(d->c, d->dtype);
  const int M = w.kp, N = d->kh * d->kw * w.cp;
  const long R = (long)d->n * d->ho * d->wo;
  w.nw = !w.sp && nw_path(d);
  if (w.nw) {
    w.splits = nwgrad_splits(d);
  } else {
    const int BK = b16 ? 64 : 16;
    // Cout <= 32 (the 19-class convs, padded to 32): a 32-row tile (register-staged) instead of
    // half a 64-row one
    w.bm = b16 ? (M <= 32 && N > 64 ? 32 : (M <= 64 ? 64 : 128)) : 64;
    w.bn = b16 ? (N <= 64 ? 64 : 128) : 64;
    const long tiles = (long)rt_cdiv(M, w.bm) * rt_cdiv(N, w.bn);
    const long nk = (R + BK - 1) / BK;
    // WGRAD split-K: enough (M/BM)*(N/BN)*splits workgroups to fill 256 CUs ~2x, each split at
    // least 8 K-tiles; fp32 partial slabs summed (and channel-unpadded) by split_reduce_kernel --
    // deterministic, no atomics.
    // narrow outputs (<= 32 rows of Cout: the 19-class convs) stream far more pixels per tile:
    // ~6 groups per CU hide more of the gather latency (DeepLab ASPP 304 -> 226 us, FFM 147 ->
    // 125).  Wide grids that fill only 432 of a round's 512 slots (DeepLab layer4 3x3, 144
    // tiles x 3) take ~2 full rounds of splits instead when every split keeps >= 64 K-tiles
    // (373 -> 325 us); short reductions (BiSeNet layer4, 64 K-tiles) would pay it in slab traffic.
    long want = std::max<long>(1, (w.bm <= 64 && M <= 32 ? 1536 : kWgradWant) / tiles);
    if (!(w.bm <= 64 && M <= 32) && tiles >= 64 && tiles * want < 480) {
      const long w2 = 1024 / tiles;
      if (tiles * w2 >= 922 && nk / w2 >= 64) want = w2;
    }
    want = std::min<long>(want, std::max<long>(1, nk / 8));
    want = std::min<long>(want, 256);
    w.tps = (int)((nk + want - 1) / want);
    w.splits = (int)((nk + w.tps - 1) / w.tps);
    w.xp_bytes = w.cp != d->c ? al256((size_t)d->n * d->h * d->w * w.cp * es) : 0;
  }
  w.slab_bytes = al256((size_t)w.splits * M * N * 4);
  w.dyp_bytes = w.kp != d->k ? al256((size_t)R * w.kp * es) : 0;
  w.colsum_bytes = al256((size_t)kColsumRB * d->k * 4);
  if (w.sp) {
    w.x4_bytes = sp_x4_bytes(d0);
    w.dws_bytes = al256((size_t)d->k * d->kh * d->kw * 8 * 4);
  } else if (pwn_wgrad_ok(d0)) {
    w.pwn_bytes = al256((size_t)pwn_blocks(d0) * (d0->k * d0->c + d0->k) * 4);
  }
  return w;
}

extern "C" size_t rtsds_conv2d_wgrad_workspace(const rtsds_conv_desc* d) {
  return pooled_1x1(d) ? 0 : wgrad_plan(d).total();
}

static int wgrad_impl(const rtsds_conv_desc* d0, const void* x, const void* dy, float* dw, float* dbias, int accumulate,
                      void* ws, size_t ws_bytes, rtsds_split_reduce_desc* pending, void* stream) {
  int e = check_desc(d0);
  if (e) return e;
  const bool x_padded = (accumulate & RTSDS_INPUT_PADDED) != 0;
  accumulate &= ~RTSDS_INPUT_PADDED;
  if (x_padded && (pooled_1x1(d0) || (!sp_path(d0) && pad_c(d0->c, d0->dtype) == d0->c))) return RTSDS_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (pooled_1x1(d0)) return pooled_wgrad(d0, x, dy, dw, dbias, accumulate ? 1 : 0, st);
  const WgradPlan pl = wgrad_plan(d0);
  if (ws_bytes < pl.total()) return RTSDS_ERR_WORKSPACE;
  if (pl.pwn_bytes) {
    const long P = (long)d0->n * d0->h * d0->w;
    const int nb = pwn_blocks(d0), per = (int)((P + nb - 1) / nb), no = d0->k * d0->c + d0->k;
    const int ldx = x_padded ? pad_c(d0->c, d0->dtype) : d0->c;
    float* part = (float*)ws;
    DISPATCH_T(d0->dtype, hipLaunchKernelGGL(pwn_wgrad_part_kernel<T>, dim3(nb), dim3(256), 0, st, (const T*)dy, (const T*)x, part,
                                             P, d0->k, d0->c, ldx, per));
    hipLaunchKernelGGL(pwn_wgrad_final_kernel, dim3(no), dim3(64), 0, st, (const float*)part, dw, dbias, nb, d0->k, d0->c,
                       accumulate ? 1 : 0);
    RET_LAUNCH();
  }
  const bool sp = pl.sp;
  const rtsds_conv_desc& dv = pl.g;
  char* slab = (char*)ws;
  char* dyp = slab + pl.slab_bytes;
  char* xp = dyp + pl.dyp_bytes;
  float* part = (float*)(xp + pl.xp_bytes);
  char* x4 = (char*)part + pl.colsum_bytes;
  float* dws = (float*)(x4 + pl.x4_bytes);  // superpixel path: dW' [k][kh][kwp][8] before the unpack
  const long R = (long)d0->n * d0->ho * d0->wo;
  rtsds_conv_desc d = dv;
  const void* dyk = dy;
  if (sp && !x_padded) {  // RTSDS_INPUT_PADDED: x already is the 4-channel superpixel image
    sp_pad4(d0, x, x4, st);
    x = x4;
  }
  // bf16 bias gradient of a narrow (k % 8, k <= 256) padded dY: the padded copy and the bias
  // column-sum partials in one pass (pad_colsum_kernel)
  const int crb = (int)std::max<long>(1, std::min<long>(kColsumRB, R / 64));
  const bool fused_colsum = dbias && pl.kp != d.k && d0->dtype == RTSDS_BF16 && d0->k % 8 != 0 && d0->k <= 256;
  if (pl.kp != d.k) {
    if (fused_colsum)
      hipLaunchKernelGGL(pad_colsum_kernel<bf16>, dim3(crb), dim3(256), 0, st, (const bf16*)dy, (bf16*)dyp, part, R, d.k, pl.kp);
    else if ((e = pad_any(d.dtype, dy, dyp, R, d.k, pl.kp, st)))
      return e;
    dyk = dyp;
    d.k = pl.kp;
  }
  if (!sp && pl.cp != d.c) {
    if (!x_padded) {  // RTSDS_INPUT_PADDED: x already has the padded channel pitch
      if ((e = pad_any(d.dtype, x, xp, (long)d.n * d.h * d.w, d.c, pl.cp, st))) return e;
      x = xp;
    }
    d.c = pl.cp;
  }
  ConvArgs p = make_args(&d);
  p.a = dyk; p.b = x; p.bias = nullptr; p.act = 0;
  p.M = d.k;
  p.N = d.kh * d.kw * d.c;
  p.K = (int)R;
  p.tiles_per_split = pl.tps;
  p.split_stride = (long)p.M * p.N;
  p.out = slab;
  if (pl.nw) {  // (dyk: 32-channel pitch; the slab rows co >= k stay unwritten)
    rtsds_conv_desc dn = d;
    dn.k = d0->k;
    nwgrad(&dn, x, dyk, (float*)slab, st);
  } else {
    DISPATCH_T(d.dtype, wgrad_launch<T>(p, pl.bm, pl.bn, pl.splits, st));
  }
  if (sp) {
    const int nv = dv.k * dv.kh * dv.kw * 2;
    hipLaunchKernelGGL(split_reduce_kernel<4>, dim3(std::min(8192, (nv + 63) / 64)), dim3(256), 0, st, (const float*)slab, dws,
                       nv, 2, fastdiv_make(2), 8, p.split_stride, pl.splits, 0);
    const int n = d0->k * d0->kh * d0->kw * 3;
    hipLaunchKernelGGL(sp_unpack_dw_kernel, dim3(rt_cdiv(n, 256)), dim3(256), 0, st, (const float*)dws, dw, d0->k, d0->kh,
                       d0->kw, dv.kw, accumulate);
  } else {
    const int V = d0->c % 4 == 0 ? 4 : 1, cv = d0->c / V;
    const int nv = d0->k * d0->kh * d0->kw * cv;
    const int blocks = std::min(8192, (nv + 63) / 64);
    if (pending && V == 4) {  // the caller reduces it later, batched (rtsds_split_reduce_many)
      pending->slab = (const float*)slab;
      pending->dw = dw;
      pending->slab_stride = p.split_stride;
      pending->nv = nv;
      pending->cv = cv;
      pending->cp = pl.cp;
      pending->splits = pl.splits;
      pending->accumulate = accumulate ? 1 : 0;
    } else if (V == 4)
      hipLaunchKernelGGL(split_reduce_kernel<4>, dim3(blocks), dim3(256), 0, st, (const float*)slab, dw, nv, cv, fastdiv_make(cv),
                         pl.cp, p.split_stride, pl.splits, accumulate);
    else
      hipLaunchKernelGGL(split_reduce_kernel<1>, dim3(blocks), dim3(256), 0, st, (const float*)slab, dw, nv, cv, fastdiv_make(cv),
                         pl.cp, p.split_stride, pl.splits, accumulate);
  }
  if (dbias) {
    const int k = d0->k;
    const int rb = crb;
    const bool b16 = d0->dtype == RTSDS_BF16;
    if (fused_colsum)
      ;  // partials already written by pad_colsum_kernel
    else if (b16 && k % 8 == 0)
      hipLaunchKernelGGL((colsum_part_kernel<bf16, 8>), dim3(rb, rt_cdiv(k, 2048)), dim3(256), 0, st, (const bf16*)dy, part, R, k);
    else if (b16)
      hipLaunchKernelGGL((colsum_part_kernel<bf16, 1>), dim3(rb, rt_cdiv(k, 256)), dim3(256), 0, st, (const bf16*)dy, part, R, k);
    else if (k % 4 == 0)
      hipLaunchKernelGGL((colsum_part_kernel<float, 4>), dim3(rb, rt_cdiv(k, 1024)), dim3(256), 0, st, (const float*)dy, part, R, k);
    else
      hipLaunchKernelGGL((colsum_part_kernel<float, 1>), dim3(rb, rt_cdiv(k, 256)), dim3(256), 0, st, (const float*)dy, part, R, k);
    hipLaunchKernelGGL(colsum_final_kernel, dim3(k), dim3(64), 0, st, (const float*)part, dbias, rb, k, accumulate);
  }
  RET_LAUNCH();
}

extern "C" int rtsds_conv2d_wgrad(const rtsds_conv_desc* d0, const void* x, const void* dy, float* dw,
                                  float* dbias, int accumulate, void* ws, size_t ws_bytes, void* stream) {
  return wgrad_impl(d0, x, dy, dw, dbias, accumulate, ws, ws_bytes, nullptr, stream);
}
extern "C" int rtsds_conv2d_wgrad_deferred(const rtsds_conv_desc* d0, const void* x, const void* dy, float* dw,
                                           float* dbias, int accumulate, void* ws, size_t ws_bytes,
                                           rtsds_split_reduce_desc* pending, void* stream) {
  if (!pending) return RTSDS_ERR_SHAPE;
  pending->nv = 0;
  return wgrad_impl(d0, x, dy, dw, dbias, accumulate, ws, ws_bytes, pending, stream);
}
