// Direct MFMA convolution for the 3-channel stride-2 image convs: the ResNet stem 7x7 s2 p3
// (build_contextpath.py via torchvision conv1; deeplabv2.py:106) and the spatial path's first
// ConvBlock 3x3 s2 p1 (build_bisenet.py:9-14, 21), 64 output channels, forward only (the image
// needs no data gradient; the weight gradient stays on the implicit GEMM's superpixel path, or --
// when the conv feeds a train-mode BatchNorm -- runs here with that BatchNorm's backward apply
// fused in: imgconv_bn_wgrad_kernel, below).
//
// These convs are epilogue-bound, not MFMA-bound: 2 x 3.6-13 GFLOP against a 134 MB output at bs 8
// 1024x512.  As an implicit GEMM each 128-row tile ran 2-7 K-steps behind a register-staged
// gather, then a full epilogue -- 73 / 112 us per launch (30 % of the HBM bound).  Here a
// workgroup owns a 4 x 64 output tile with all 64 channels:
//  * the tile's input rows are staged ONCE into LDS as 16-B "superpixels" (two horizontally
//    adjacent pixels of the 4-channel-padded image, conv_host.h sp_path): (2*4 + kh - 2) rows x
//    (64 + (kw+1)/2 - 1) superpixels, one buffer-resource LDS-DMA per 16 B, padding zero-filled
//    by the DMA (offsets past num_records);
//  * with odd padding, taps s = 2p - 1 + q of output column ow read superpixel ow - (pw+1)/2 + p,
//    so in superpixel units the conv is stride 1 horizontally: an A fragment (16 pixels x one
//    superpixel of K) is one ds_read_b128 of 16 consecutive LDS superpixels;
//  * wave w computes output channels 16w..16w+15 for all 256 pixels: its B fragments (kh *
//    (kw+1)/2 superpixel slots of 8 weights, zero for the padding channel / taps outside the
//    kernel) are built once in registers from the [64][kh][kw][3] weights (DMA-staged raw
//    into LDS beside the input rows) -- no repack launch;
//  * K order (row tap, superpixel, 8 elements) in 32-deep MFMA steps, identical to the
//    superpixel GEMM's BK = 32 K-steps, so the accumulators match it bit for bit;
//  * epilogue: bias or eval-BN scale / shift, activation, the following BatchNorm's per-tile
//    (count, mean, M2) from the fp32 values, and 8-B stores of 4 channels per pixel straight
//    from the (transposed) accumulators.
// Inference also has a variant with the stem's 3x3 stride-2 max pool in the epilogue
// (imgconv_pool_kernel): the full-resolution activation is never written.
#include "conv_host.h"
#include "bn_dev.h"

template <int N> RT_DEV void wait_vmcnt_img() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// Sum over the 16 lanes of a DPP row (every lane of the row ends with the total): quad_perm
// [1,0,3,2], [2,3,0,1], then row_half_mirror, row_mirror -- VALU ops, no LDS round trip.
RT_DEV float row16_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x141, 0xF, 0xF, false));
  v += __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), 0x140, 0xF, 0xF, false));
  return v;
}
// 8-B buffer store; an offset past num_records is dropped by the hardware
RT_DEV void store8(rsrc_t r, bf16x4 v, int off) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, v), r, off, 0, 0);
#endif
}

// Activation of the epilogues.  ACT >= 0: the activation fixed at compile time (RTSDS_ACT_NONE /
// RTSDS_ACT_RELU, the ones the image convs run with), ACT < 0: chosen per launch.  With the
// runtime choice every value paid the uniform compare-and-branch chain of the switch (~200
// scalar branches per tile in the pooled stem); the fixed forms are one VALU op or none.
template <int ACT>
RT_DEV float img_act(float t, int act) {
  const int a = ACT >= 0 ? ACT : act;
  if (a == RTSDS_ACT_RELU) return fmaxf(t, 0.f);
  if (a == RTSDS_ACT_LEAKY) return t > 0.f ? t : 0.2f * t;
  if (a == RTSDS_ACT_SIGMOID) return 1.f / (1.f + expf(-t));
  return t;
}
static int img_act_variant(int act) { return act == RTSDS_ACT_NONE ? 0 : act == RTSDS_ACT_RELU ? 1 : -1; }

namespace {
constexpr int kTH = 4, kTW = 64;   // output tile rows x columns (all 64 channels)
constexpr int kCo = 64;            // output channels (4 waves x 16)
}  // namespace

struct ImgArgs {
  const bf16* x4;      // [n][h][w][4], channel 3 zero
  const bf16* wt;      // [64][kh][kw][3]
  const float* bias;   // [64] or null (eval fold: shift)
  const float* scale;  // [64] or null (eval fold)
  bf16* y;             // [n][ho][wo][64]
  float* stats;        // [64][tiles][4] (count, mean, M2, 0) or null
  int n, h, w, ho, wo, ph, pw, act;
  int tiles, per;      // tiles, tiles per workgroup (a contiguous run)
};

// WP x WC waves: WP pixel halves (8 groups each) x WC channel slices of 64 / WC
template <int KH, int KW, int WP, int ACT>
__global__ void __launch_bounds__(256, (KH == 7 || WP != 1) ? 2 : 3) imgconv_fwd_kernel(const ImgArgs P) {
  constexpr int WC = 4 / WP, GP = 16 / WP, NCB = kCo / WC / 16;  // pixel groups, 16-channel blocks per wave
  constexpr int KWP = (KW + 1) / 2;          // superpixels per row tap
  constexpr int NQ = KH * KWP;               // superpixel slots of K
  constexpr int KS = (NQ + 3) / 4;           // 32-deep MFMA steps
  constexpr int NR = 2 * kTH + KH - 2;       // staged input rows
  constexpr int NC = kTW + KWP - 1;          // staged superpixels per row
  constexpr int NP = NR * NC;                // 16-B pieces
  constexpr int NI = (NP + 63) / 64;         // DMA wave-instructions per tile
  constexpr int NIW = (NI + 3) / 4;          // per wave
  constexpr int W_EL = kCo * KH * KW * 3;    // raw weights
  constexpr int NWI = (W_EL * 2 + 1023) / 1024, NWIW = (NWI + 3) / 4;
  constexpr int A_BYTES = NI * 1024;
  __shared__ __attribute__((aligned(16))) unsigned char lds[NWI * 1024 + 2 * A_BYTES];
  unsigned char* const abuf = lds + NWI * 1024;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bid;
  {  // XCD-aware bijective remap: the workgroups of one XCD take adjacent runs of tiles
    const int nwg = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  }
  const int t0 = bid * P.per, t1 = min(P.tiles, t0 + P.per);
  const int tw_n = (P.wo + kTW - 1) / kTW, th_n = (P.ho + kTH - 1) / kTH;
  const int spw = P.w >> 1;                  // superpixels per image row
  const int pwp = (P.pw + 1) >> 1;
  const rsrc_t rx = make_rsrc(P.x4, P.n * P.h * P.w * 8);
  const rsrc_t ry = make_rsrc(P.y, P.n * P.ho * P.wo * kCo * 2);
  auto tile_xy = [&](int t, int& img, int& oh0, int& ow0) {
    img = t / (th_n * tw_n);
    const int rem = t - img * th_n * tw_n, trow = rem / tw_n;
    oh0 = trow * kTH;
    ow0 = (rem - trow * tw_n) * kTW;
  };
  // input rows of tile t (zero outside the image) -> A buffer b
  auto issue = [&](int t, int b) {
    int img, oh0, ow0;
    tile_xy(t, img, oh0, ow0);
    const int ih0 = 2 * oh0 - P.ph, j0 = ow0 - pwp;
#pragma unroll
    for (int i = 0; i < NIW; ++i) {
      const int ins = wave + 4 * i;
      if (ins < NI) {
        const int piece = ins * 64 + lane;
        const int row = piece / NC, col = piece - row * NC;
        const int ih = ih0 + row, j = j0 + col;
        const bool ok = piece < NP && (unsigned)ih < (unsigned)P.h && (unsigned)j < (unsigned)spw;
        buf_lds16(rx, abuf + b * A_BYTES + ins * 1024, ok ? ((img * P.h + ih) * spw + j) * 16 : (int)0x80000000, 0);
      }
    }
  };

  // ---- raw weights (once per workgroup), then the first tile's input
  const rsrc_t rw = make_rsrc(P.wt, W_EL * 2);
#pragma unroll
  for (int i = 0; i < NWIW; ++i) {
    const int ins = wave + 4 * i;
    if (ins < NWI) buf_lds16(rw, lds + ins * 1024, (ins * 64 + lane) * 16, 0);
  }
  issue(t0, 0);
  const int fr = lane & 15, fc = lane >> 4;
  const int wp = wave / WC, c0 = (wave % WC) * (kCo / WC);  // pixel half, first channel
  // this lane's output channels: c0 + 16 cb + 4 (lane >> 4) + e
  float bv[NCB][4], sv[NCB][4];
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int ch = c0 + 16 * cb + 4 * fc + e;
      bv[cb][e] = P.bias ? P.bias[ch] : 0.f;
      sv[cb][e] = P.scale ? P.scale[ch] : 1.f;
    }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // ---- weight fragments (the MFMA's A operand: rows = channels c0 + 16 cb + (lane & 15), K
  // slot q = 4 ks + (lane >> 4)) and the per-slot LDS offsets of the pixel fragments
  const bf16* ws = (const bf16*)lds;
  bf16x8 fw[NCB][KS];
  int koff[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int q = 4 * ks + fc;
    const int r = q / KWP, p = q - r * KWP;
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb) {
      const int n = c0 + 16 * cb + fr;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int s = 2 * p - 1 + (e >> 2), ch = e & 3;
        bf16 v = (bf16)0.f;
        if (q < NQ && ch < 3 && s >= 0 && s < KW) v = ws[((n * KH + r) * KW + s) * 3 + ch];
        fw[cb][ks][e] = v;
      }
    }
    // slots past NQ carry zero weights: read any staged (finite) superpixel for them
    const int qq = q < NQ ? q : 0;
    koff[ks] = ((qq / KWP) * NC + (qq % KWP) + fr) * 16;
  }
  auto act_f = [&](float t) { return img_act<ACT>(t, P.act); };

  float rn = 0.f, rmean[NCB][4], rm2[NCB][4];  // running BatchNorm statistics of this wave's channels
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int e = 0; e < 4; ++e) rmean[cb][e] = rm2[cb][e] = 0.f;
  for (int t = t0; t < t1; ++t) {
    const int b = (t - t0) & 1;
    // tile t's input landed (the GP * NCB newest VMEM ops are the previous tile's output stores,
    // issued after this DMA), every wave is done with the other buffer: refill it
    if (t > t0) wait_vmcnt_img<GP * NCB>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 1 < t1) issue(t + 1, b ^ 1);
    int img, oh0, ow0;
    tile_xy(t, img, oh0, ow0);

    // ---- this wave's GP pixel groups (group g = GP wp + i: tile row g / 4, columns 16 (g % 4)
    // + (lane & 15)) x NCB channel blocks: C^T = W x X^T, so each lane ends with 4 consecutive
    // channels of one pixel per block
    f32x4 acc[GP][NCB];
#pragma unroll
    for (int i = 0; i < GP; ++i)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) acc[i][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned char* ab = abuf + b * A_BYTES;
    // group-major with one group of look-ahead: group i + 1's KS fragments are read before
    // group i's MFMAs (two register sets; the scheduling barriers keep the reads where they
    // are placed -- left alone the scheduler hoisted all GP x KS reads and spilled, and reading
    // each group right before its MFMAs exposed the LDS latency once per group)
    auto rdg = [&](int i, bf16x8* fa) {
      const int g = GP * wp + i;
      const int goff = ((2 * (g >> 2)) * NC + (g & 3) * 16) * 16;
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) fa[ks] = *(const bf16x8*)(ab + koff[ks] + goff);
    };
    bf16x8 fa0[KS], fa1[KS];
    rdg(0, fa0);
#pragma unroll
    for (int i = 0; i < GP; ++i) {
      bf16x8* fa = (i & 1) ? fa1 : fa0;
      if (i + 1 < GP) rdg(i + 1, (i & 1) ? fa0 : fa1);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
          acc[i][cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[cb][ks], fa[ks], acc[i][cb], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }

    // ---- epilogue: acc[i][cb][e] = C[channel c0 + 16 cb + 4 (lane >> 4) + e][pixel]
    const int vrows = min(kTH, P.ho - oh0), vcols = min(kTW, P.wo - ow0);
#pragma unroll
    for (int i = 0; i < GP; ++i)
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][cb][e] = fmaf(acc[i][cb][e], sv[cb][e], bv[cb][e]);
    auto pix_ok = [&](int g) { return (g >> 2) < vrows && (g & 3) * 16 + fr < vcols; };
    if (P.stats) {
      // per-channel (count, mean, M2) over the valid pixels of this wave's part of the tile,
      // exact two-pass: lane sums over its GP pixels, then over the 16 lanes holding the same
      // channels; merged (Chan) into the workgroup's running statistics
      int nv = 0;
#pragma unroll
      for (int i = 0; i < GP; ++i) {
        const int g = GP * wp + i;
        nv += (g >> 2) < vrows ? max(0, min(16, vcols - (g & 3) * 16)) : 0;
      }
      const float cnt = (float)nv;
      const float rn1 = rn + cnt;
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        float mean[4];
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
          float sacc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int i = 0; i < GP; ++i) {
            const bool ok = pix_ok(GP * wp + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float d = pass == 0 ? acc[i][cb][e] : acc[i][cb][e] - mean[e];
              if (ok) sacc[e] += pass == 0 ? d : d * d;
            }
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            sacc[e] = row16_sum(sacc[e]);
            if (pass == 0) mean[e] = nv ? sacc[e] / cnt : 0.f;
          }
          if (pass == 1 && nv) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              if (rn == 0.f) {
                rmean[cb][e] = mean[e];
                rm2[cb][e] = sacc[e];
              } else {
                const float dd = mean[e] - rmean[cb][e];
                rmean[cb][e] += dd * (cnt / rn1);
                rm2[cb][e] += sacc[e] + dd * dd * (rn * cnt / rn1);
              }
            }
          }
        }
      }
      rn = rn1;
    }
    // ---- 8-B stores of 4 channels per pixel; rows / columns past the output fall past
    // num_records and are dropped (every wave issues exactly GP * NCB stores per tile)
#pragma unroll
    for (int i = 0; i < GP; ++i) {
      const int g = GP * wp + i;
      const int oh = oh0 + (g >> 2), ow = ow0 + (g & 3) * 16 + fr;
      const bool ok = pix_ok(g);
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb) {
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (bf16)act_f(acc[i][cb][e]);
        const int off = ok ? (((img * P.ho + oh) * P.wo + ow) * kCo + c0 + 16 * cb + 4 * fc) * 2 : (int)0x80000000;
        store8(ry, o, off);
      }
    }
  }
  if (P.stats && fr == 0) {  // partial-statistics row WP bid + wp: [channel][row][4]
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int e = 0; e < 4; ++e)
        *(f32x4*)(P.stats + ((long)(c0 + 16 * cb + 4 * fc + e) * gridDim.x * WP + WP * bid + wp) * 4) =
            f32x4{rn, rmean[cb][e], rm2[cb][e], 0.f};
  }
}

// ---- conv + eval BatchNorm (folded scale / shift) + activation + MaxPool2d(3, 2, pp) (the
// ResNet stem at inference: build_contextpath.py via torchvision resnet; deeplabv2.py:106-110,
// ceil mode).  A tile is PH pooled rows x 31 pooled columns: conv rows 2 po0 - pp .. + 2 PH and
// 64 conv columns from 2 pc0 - pp (the 31 windows need 63 of them), (2 PH + 1) x 4 MFMA pixel
// groups per wave (4 waves x 16 channels).  Each conv value is rounded to bf16 exactly as the conv kernel stores
// it; the window maximum is taken vertically in registers and horizontally across lanes
// (ds_bpermute), conv positions outside the conv output are skipped (padding / ceil-mode
// windows), so the result equals imgconv_fwd_kernel followed by maxpool_fwd_k3 bit for bit.
namespace {
constexpr int kPW = 31;  // pooled columns per tile
}
struct ImgPoolArgs {
  const bf16* x4;
  const bf16* wt;
  const float* shift;
  const float* scale;
  bf16* y;             // [n][hp][wp][64]
  int n, h, w, ho, wo, ph, pw, act;
  int hp, wp, pp;      // pooled output size, pool padding
  int tiles, per;
};
template <int KH, int KW, int PH, int ACT>
__global__ void __launch_bounds__(256, 2) imgconv_pool_kernel(const ImgPoolArgs P) {
  constexpr int KWP = (KW + 1) / 2, NQ = KH * KWP, KS = (NQ + 3) / 4;
  constexpr int CR = 2 * PH + 1, NG = 4 * CR;  // conv rows, pixel groups per tile
  constexpr int NR = 2 * (CR - 1) + KH;      // input rows of the CR conv rows (stride 2)
  constexpr int NC = 64 + KWP - 1;
  constexpr int NP = NR * NC, NI = (NP + 63) / 64, NIW = (NI + 3) / 4;
  constexpr int W_EL = kCo * KH * KW * 3;
  constexpr int NWI = (W_EL * 2 + 1023) / 1024, NWIW = (NWI + 3) / 4;
  constexpr int A_BYTES = NI * 1024;
  constexpr int NST = 4 * PH;                // output store instructions per wave and tile
  __shared__ __attribute__((aligned(16))) unsigned char lds[NWI * 1024 + 2 * A_BYTES];
  unsigned char* const abuf = lds + NWI * 1024;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int bid;
  {
    const int nwg = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  }
  const int t0 = bid * P.per, t1 = min(P.tiles, t0 + P.per);
  const int tw_n = (P.wp + kPW - 1) / kPW, th_n = (P.hp + PH - 1) / PH;
  const int spw = P.w >> 1, pwp = (P.pw + 1) >> 1;
  const rsrc_t rx = make_rsrc(P.x4, P.n * P.h * P.w * 8);
  const rsrc_t ry = make_rsrc(P.y, P.n * P.hp * P.wp * kCo * 2);
  auto tile_xy = [&](int t, int& img, int& po, int& pc0) {  // po: the tile's first pooled row
    img = t / (th_n * tw_n);
    const int rem = t - img * th_n * tw_n, tr = rem / tw_n;
    po = tr * PH;
    pc0 = (rem - tr * tw_n) * kPW;
  };
  auto issue = [&](int t, int b) {
    int img, po, pc0;
    tile_xy(t, img, po, pc0);
    const int cr0 = 2 * po - P.pp, cc0 = 2 * pc0 - P.pp;
    const int ih0 = 2 * cr0 - P.ph, j0 = cc0 - pwp;
#pragma unroll
    for (int i = 0; i < NIW; ++i) {
      const int ins = wave + 4 * i;
      if (ins < NI) {
        const int piece = ins * 64 + lane;
        const int row = piece / NC, col = piece - row * NC;
        const int ih = ih0 + row, j = j0 + col;
        const bool ok = piece < NP && (unsigned)ih < (unsigned)P.h && (unsigned)j < (unsigned)spw;
        buf_lds16(rx, abuf + b * A_BYTES + ins * 1024, ok ? ((img * P.h + ih) * spw + j) * 16 : (int)0x80000000, 0);
      }
    }
  };
  const rsrc_t rw = make_rsrc(P.wt, W_EL * 2);
#pragma unroll
  for (int i = 0; i < NWIW; ++i) {
    const int ins = wave + 4 * i;
    if (ins < NWI) buf_lds16(rw, lds + ins * 1024, (ins * 64 + lane) * 16, 0);
  }
  if (t0 < t1) issue(t0, 0);
  const int fr = lane & 15, fc = lane >> 4;
  const int nb = wave * 16 + 4 * fc;         // this lane's output channels nb .. nb + 3
  float bv[4], sv[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bv[e] = P.shift ? P.shift[nb + e] : 0.f;
    sv[e] = P.scale ? P.scale[nb + e] : 1.f;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  const bf16* ws = (const bf16*)lds;
  bf16x8 fw[KS];
  int koff[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    const int q = 4 * ks + fc;
    const int r = q / KWP, p = q - r * KWP;
    const int n = wave * 16 + fr;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int s = 2 * p - 1 + (e >> 2), ch = e & 3;
      bf16 v = (bf16)0.f;
      if (q < NQ && ch < 3 && s >= 0 && s < KW) v = ws[((n * KH + r) * KW + s) * 3 + ch];
      fw[ks][e] = v;
    }
    const int qq = q < NQ ? q : 0;
    koff[ks] = ((qq / KWP) * NC + (qq % KWP) + fr) * 16;
  }
  auto act_f = [&](float t) { return img_act<ACT>(t, P.act); };
  // window maximum with maxpool_fwd_k3's rule (a NaN wins)
  auto mx = [](float best, float f) { return (f > best || (f != f && best == best)) ? f : best; };

  for (int t = t0; t < t1; ++t) {
    const int b = (t - t0) & 1;
    if (t > t0) wait_vmcnt_img<NST>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 1 < t1) issue(t + 1, b ^ 1);
    int img, po, pc0;
    tile_xy(t, img, po, pc0);
    const int cr0 = 2 * po - P.pp, cc0 = 2 * pc0 - P.pp;

    // NG pixel groups: conv row g / 4, columns 16 (g % 4) + (lane & 15)
    f32x4 acc[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
    const unsigned char* ab = abuf + b * A_BYTES;
    // (no look-ahead here, unlike imgconv_fwd_kernel: its second fragment set costs this kernel
    // a workgroup per CU -- 155 -> 194 VGPRs, eval stem 70 -> 78 us)
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int goff = ((2 * (g >> 2)) * NC + (g & 3) * 16) * 16;
      bf16x8 fa[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) fa[ks] = *(const bf16x8*)(ab + koff[ks] + goff);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[ks], fa[ks], acc[g], 0, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
    }
    // the conv outputs as stored by the conv kernel (folded BN, activation, bf16 rounding), in
    // place; a NaN anywhere in the wave's tile sends the wave down the exact NaN-ordered path
    float probe = 0.f;
#pragma unroll
    for (int g = 0; g < NG; ++g)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[g][e] = (float)(bf16)act_f(fmaf(acc[g][e], sv[e], bv[e]));
        probe = fmaf(acc[g][e], 0.f, probe);  // NaN iff some value is NaN or infinite
      }
    const bool exact = __builtin_amdgcn_ballot_w64(probe != probe) != 0;  // wave-uniform
#pragma unroll
    for (int pr = 0; pr < PH; ++pr) {
      // vertical maxima (invalid conv positions skipped: -inf)
      float vm[4][4];
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) {
        const int cc = cc0 + cg * 16 + fr;
        const bool cok = (unsigned)cc < (unsigned)P.wo;
#pragma unroll
        for (int e = 0; e < 4; ++e) vm[cg][e] = -INFINITY;
        if (exact) {
          bool any = false;
#pragma unroll
          for (int tr = 0; tr < 3; ++tr) {
            const int cr = cr0 + 2 * pr + tr;
            if ((unsigned)cr < (unsigned)P.ho && cok) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float v = acc[(2 * pr + tr) * 4 + cg][e];
                vm[cg][e] = any ? mx(vm[cg][e], v) : v;
              }
              any = true;
            }
          }
        } else {  // no NaN: compare-and-select from -inf gives the same maximum (and the same zero sign)
#pragma unroll
          for (int tr = 0; tr < 3; ++tr) {
            const int cr = cr0 + 2 * pr + tr;
            if ((unsigned)cr < (unsigned)P.ho) {
#pragma unroll
              for (int e = 0; e < 4; ++e) {
                const float v = cok ? acc[(2 * pr + tr) * 4 + cg][e] : -INFINITY;
                vm[cg][e] = v > vm[cg][e] ? v : vm[cg][e];
              }
            }
          }
        }
      }
      // horizontal: pooled column j = 8 cg + fr / 2 (even lanes) covers local conv columns
      // fr, fr + 1, fr + 2 of group cg (fr + 2 = 16: lane 0 of group cg + 1)
#pragma unroll
      for (int cg = 0; cg < 4; ++cg) {
        const int l1 = (lane & ~15) | ((fr + 1) & 15), l2 = (lane & ~15) | ((fr + 2) & 15);
        float o[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float a1 = __shfl(vm[cg][e], l1, 64);
          const float a2s = __shfl(vm[cg][e], l2, 64), a2n = __shfl(vm[cg < 3 ? cg + 1 : cg][e], l2, 64);
          const float a2 = fr + 2 < 16 ? a2s : a2n;  // (the selection is the reader's)
          // window order: left column, then middle, then right (skip -inf = no valid position)
          float best = vm[cg][e];
          if (exact) {
            best = a1 == -INFINITY ? best : (best == -INFINITY ? a1 : mx(best, a1));
            best = a2 == -INFINITY ? best : (best == -INFINITY ? a2 : mx(best, a2));
          } else {
            best = a1 > best ? a1 : best;
            best = a2 > best ? a2 : best;
          }
          o[e] = best;
        }
        const int pc = pc0 + cg * 8 + (fr >> 1), pry = po + pr;
        const bool ok = (fr & 1) == 0 && cg * 8 + (fr >> 1) < kPW && pry < P.hp && pc < P.wp;
        bf16x4 ov;
#pragma unroll
        for (int e = 0; e < 4; ++e) ov[e] = (bf16)o[e];
        store8(ry, ov, ok ? (((img * P.hp + pry) * P.wp + pc) * kCo + nb) * 2 : (int)0x80000000);
      }
    }
  }
}

// ---- host -------------------------------------------------------------------------------
// The superpixel geometry of conv_host.h's sp_path with 64 output channels and a 7x7 or 3x3 kernel.
bool imgconv_ok(const rtsds_conv_desc* d) {
  if (!(d->dtype == RTSDS_BF16 && d->c == 3 && d->k == kCo && d->sh == 2 && d->sw == 2 && d->dh == 1 && d->dw == 1 &&
        (d->pw & 1) == 1 && (d->w & 1) == 0))
    return false;
  if (!((d->kh == 7 && d->kw == 7) || (d->kh == 3 && d->kw == 3))) return false;
  return (long)d->n * d->h * d->w * 8 < (1L << 31) && (long)d->n * d->ho * d->wo * kCo * 2 < (1L << 31);
}
// Wave layouts (measured, tools/ab_imgconv.sh, bs 8 1024x512): the 7x7 stem in 2 pixel halves x
// 2 channel halves (71.5 / 57 us train / eval vs 74 / 60.5 in 4 channel quarters); the 3x3
// spatial-path conv in channel quarters with the statistics epilogue (54 vs 58 us) and pixel
// halves without it (41.5 vs 45.8 us).
template <int ACT>
static const void* img_kernel_act(int kh, bool stats) {
  if (kh == 7) return (const void*)imgconv_fwd_kernel<7, 7, 2, ACT>;
  return stats ? (const void*)imgconv_fwd_kernel<3, 3, 1, ACT> : (const void*)imgconv_fwd_kernel<3, 3, 2, ACT>;
}
static const void* img_kernel(int kh, bool stats, int act) {
  const int v = img_act_variant(act);
  return v == 0 ? img_kernel_act<0>(kh, stats) : v == 1 ? img_kernel_act<1>(kh, stats) : img_kernel_act<-1>(kh, stats);
}
static int img_wp(int kh, bool stats) { return kh == 7 ? 2 : (stats ? 1 : 2); }
static int img_tiles(const rtsds_conv_desc* d) { return d->n * rt_cdiv(d->ho, kTH) * rt_cdiv(d->wo, kTW); }
// Persistent grid: every workgroup walks a contiguous run of `per` tiles (weights staged once,
// the next tile's input DMA in flight behind the current tile's MFMAs and stores); enough
// workgroups for the resident slots of all CUs.  Every workgroup gets >= 1 tile.
static void img_grid(const rtsds_conv_desc* d, bool stats, int& grid, int& per) {
  static int occ[3] = {0, 0, 0}, cus = 0;
  const int v = d->kh == 7 ? 2 : (stats ? 1 : 0);
  // (the activation variants share the launch bounds and register budget: ReLU's stands for all)
  if (!occ[v] && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ[v], img_kernel(d->kh, stats, RTSDS_ACT_RELU), 256, 0) != hipSuccess ||
                  occ[v] < 1))
    occ[v] = 1;
  if (!cus && (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus < 1)) cus = 256;
  const int tiles = img_tiles(d), slots = cus * occ[v];
  per = (tiles + slots - 1) / slots;
  grid = (tiles + per - 1) / per;
}
// BatchNorm partial-statistics rows of the training launch: one per workgroup and pixel part
int imgconv_tiles(const rtsds_conv_desc* d) {
  int grid, per;
  img_grid(d, true, grid, per);
  return grid * img_wp(d->kh, true);
}
void imgconv_fwd(const rtsds_conv_desc* d, const void* x4, const void* w, const float* bias, const float* scale, void* y,
                 int act, float* stats, hipStream_t st) {
  ImgArgs a;
  a.x4 = (const bf16*)x4; a.wt = (const bf16*)w; a.bias = bias; a.scale = scale; a.y = (bf16*)y; a.stats = stats;
  a.n = d->n; a.h = d->h; a.w = d->w; a.ho = d->ho; a.wo = d->wo; a.ph = d->ph; a.pw = d->pw; a.act = act;
  a.tiles = img_tiles(d);
  int grid;
  img_grid(d, stats != nullptr, grid, a.per);
  void* args[] = {&a};
  (void)hipLaunchKernel(img_kernel(d->kh, stats != nullptr, act), dim3(grid), dim3(256), args, 0, st);
}

// Pooled stem at inference (imgconv_pool_kernel): conv + folded BN + act + MaxPool2d(3, 2, pp).
bool imgconv_pool_ok(const rtsds_conv_desc* d, int hp, int wp) {
  return imgconv_ok(d) && d->kh == 7 && hp > 0 && wp > 0 && (long)d->n * hp * wp * kCo * 2 < (1L << 31);
}
void imgconv_pool_fwd(const rtsds_conv_desc* d, const void* x4, const void* w, const float* shift, const float* scale, void* y,
                      int act, int hp, int wp, int pp, hipStream_t st) {
  ImgPoolArgs a;
  a.x4 = (const bf16*)x4; a.wt = (const bf16*)w; a.shift = shift; a.scale = scale; a.y = (bf16*)y;
  a.n = d->n; a.h = d->h; a.w = d->w; a.ho = d->ho; a.wo = d->wo; a.ph = d->ph; a.pw = d->pw; a.act = act;
  a.hp = hp; a.wp = wp; a.pp = pp;
// 2 pooled rows per tile (tools/ab_pool.sh, bs 8 1024x512: 106 us vs 111 at 1 row, 155 at 3 with
// one group per CU; the separate folded conv + pool take 59 + 63 us)
static constexpr auto kImgPoolPH = 2;
  a.tiles = d->n * rt_cdiv(hp, kImgPoolPH) * rt_cdiv(wp, kPW);
  const int v = img_act_variant(act);
  const void* k = v == 0 ? (const void*)imgconv_pool_kernel<7, 7, kImgPoolPH, 0>
                : v == 1 ? (const void*)imgconv_pool_kernel<7, 7, kImgPoolPH, 1>
                         : (const void*)imgconv_pool_kernel<7, 7, kImgPoolPH, -1>;
  static int occ = 0, cus = 0;
  if (!occ && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, (const void*)imgconv_pool_kernel<7, 7, kImgPoolPH, 1>, 256, 0) != hipSuccess ||
               occ < 1))
    occ = 1;
  if (!cus && (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus < 1)) cus = 256;
  const int slots = cus * occ;
  a.per = (a.tiles + slots - 1) / slots;
  const int grid = (a.tiles + a.per - 1) / a.per;
  void* args[] = {&a};
  (void)hipLaunchKernel(k, dim3(grid), dim3(256), args, 0, st);
}

// ---- weight gradient with the following BatchNorm's backward apply fused in -----------------
// dW[co][r][s][ch] = sum_px dx[px][co] X[px + tap (r, s)][ch] where dx is the BatchNorm's data
// gradient, dx = A*g + B*(x - mean) + C (g = dy masked by the activation).  The image needs no
// data gradient, so dx had exactly one reader -- this sum -- and bn_bwd_apply wrote 134 MB per
// layer at bs 8 1024x512 for the GEMM to read back.  Here a workgroup walks the forward kernel's
// 4 x 64-pixel tiles; per tile
//  * every thread loads 8 x 16 B of g and of x (pixel tid / 8 + 32 u, channels 8 (tid % 8) ..),
//    one tile ahead of its use, forms dx with bn.hip's own expressions (bn_dev.h), rounds it to
//    bf16 as the apply pass stores it and writes it to LDS pixel-major (128-B rows; the 32-B
//    chunk c of pixel q at slot c ^ ((q >> 1) & 3): the 8 pixels a 32-lane half reads cover all
//    64 banks); pixels outside the output get dx = 0;
//  * the input rows are staged as superpixels by LDS-DMA exactly as the forward stages them
//    (double-buffered, one tile ahead);
//  * K = the tile's 256 pixels in 8 MFMA steps of 32; both operands are pixel-major in LDS and
//    read with ds_read_b64_tr_b16 (lane 16 g + 4 q + p: pixel 4 g + q, then + 16; 8-byte run p of
//    its 32-byte row -- EXEC is all ones here, every address 8-byte aligned).  An image fragment
//    is the 16 elements (two superpixels) at superpixel column + 2 j of row tap r: N block (r, j)
//    holds taps s = 4 j - 1 .. 4 j + 2; wave (wm, wn) keeps 4 / WM blocks of 16 output channels x
//    NB / WN of the N blocks in fp32 accumulators across its whole run of tiles.
// Each workgroup writes one slab already in dW's [64][kh][kw][3] order (the padding channel and
// the taps outside the kernel are simply not stored: the superpixel unpack is the store's index
// map), and the weight-gradient split reduce sums the slabs in workgroup order into dw --
// deterministic, no atomics, immediate or deferred.
struct ImgWgArgs {
  const bf16* x4;     // [n][h][w][4], channel 3 zero
  const bf16* g;      // [n][ho][wo][64] the BatchNorm's incoming gradient (before the mask)
  const bf16* xb;     // [n][ho][wo][64] the BatchNorm's input
  const float* coef;  // [A | B | C | mean | scale | shift] x 64
  float* slab;        // [workgroups][64 * kh * kw * 3]
  int n, h, w, ho, wo, ph, pw, act;
  int tiles, per;
};
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_img;
RT_DEV u32x4_img img_load16(rsrc_t r, int off) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
#else
  return u32x4_img{};
#endif
}
RT_DEV bf16x8 img_tr_frag(const unsigned char* p0, const unsigned char* p1) {
#if defined(__HIP_DEVICE_COMPILE__)
  const s16x4 t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p0);
  const s16x4 t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)p1);
  typedef __attribute__((ext_vector_type(8))) short s16x8;
  const s16x8 r = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
  return __builtin_bit_cast(bf16x8, r);
#else
  return bf16x8{};
#endif
}

template <int KH, int KW, int WN, int ACT>
__global__ void __launch_bounds__(256, 2) imgconv_bn_wgrad_kernel(const ImgWgArgs P) {
  constexpr int KWP = (KW + 1) / 2, NJ = KWP / 2, NB = KH * NJ;  // N blocks of 16 (two superpixel slots)
  static_assert(KWP % 2 == 0 && NB % WN == 0 && 4 % WN == 0, "wave layout");
  constexpr int WM = 4 / WN, CB = 4 / WM, NBW = NB / WN;
  constexpr int NR = 2 * kTH + KH - 2, NC = kTW + KWP - 1, NP = NR * NC;
  constexpr int NI = (NP + 63) / 64, NIW = (NI + 3) / 4, A_BYTES = NI * 1024;
  constexpr int DX_BYTES = kTH * kTW * kCo * 2, CF_BYTES = 6 * kCo * 4;
  constexpr int W_EL = kCo * KH * KW * 3;
  constexpr int U = kTH * kTW / 32;          // pixels per thread and tile
  // (separate arrays, and the image buffer of a tile fixed at compile time below: a transposed
  // read then provably does not alias the LDS-DMA in flight into the other image buffer, and the
  // compiler does not make it wait for that DMA)
  __shared__ __attribute__((aligned(16))) float cf[CF_BYTES / 4];
  __shared__ __attribute__((aligned(16))) unsigned char dxs[DX_BYTES];
  __shared__ __attribute__((aligned(16))) unsigned char abuf0[A_BYTES];
  __shared__ __attribute__((aligned(16))) unsigned char abuf1[A_BYTES];

  // (wave: uniform, so the per-wave tile pieces and N blocks are scalar)
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int bid;
  {  // XCD-aware bijective remap, as the forward
    const int nwg = gridDim.x, b = blockIdx.x;
    const int xcd = b & 7, q = nwg >> 3, r = nwg & 7;
    bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
  }
  const int t0 = bid * P.per, t1 = min(P.tiles, t0 + P.per);
  const int tw_n = (P.wo + kTW - 1) / kTW, th_n = (P.ho + kTH - 1) / kTH;
  const int spw = P.w >> 1, pwp = (P.pw + 1) >> 1;
  const int ybytes = P.n * P.ho * P.wo * kCo * 2;
  const rsrc_t rx = make_rsrc(P.x4, P.n * P.h * P.w * 8);
  const rsrc_t rg = make_rsrc(P.g, ybytes), rb = make_rsrc(P.xb, ybytes);
  auto tile_xy = [&](int t, int& img, int& oh0, int& ow0) {
    img = t / (th_n * tw_n);
    const int rem = t - img * th_n * tw_n, trow = rem / tw_n;
    oh0 = trow * kTH;
    ow0 = (rem - trow * tw_n) * kTW;
  };
  // input rows of tile t (zero outside the image) -> image buffer dst: imgconv_fwd_kernel's staging
  auto issue = [&](int t, unsigned char* dst) {
    int img, oh0, ow0;
    tile_xy(t, img, oh0, ow0);
    const int ih0 = 2 * oh0 - P.ph, j0 = ow0 - pwp;
#pragma unroll
    for (int i = 0; i < NIW; ++i) {
      const int ins = wave + 4 * i;
      if (ins < NI) {
        const int piece = ins * 64 + lane;
        const int row = piece / NC, col = piece - row * NC;
        const int ih = ih0 + row, j = j0 + col;
        const bool ok = piece < NP && (unsigned)ih < (unsigned)P.h && (unsigned)j < (unsigned)spw;
        buf_lds16(rx, dst + ins * 1024, ok ? ((img * P.h + ih) * spw + j) * 16 : (int)0x80000000, 0);
      }
    }
  };
  // this thread's 8 channels of pixels (tid >> 3) + 32 u of tile t: g and x, 16 B each (an offset
  // past num_records reads zeros; such pixels are zeroed again after the BatchNorm expression)
  const int cg = tid & 7, pq = tid >> 3;
  u32x4_img gv[U], xv[U];
  auto fetch = [&](int t) {
    int img, oh0, ow0;
    tile_xy(t, img, oh0, ow0);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int px = pq + 32 * u, oh = oh0 + (px >> 6), ow = ow0 + (px & 63);
      const int off = (oh < P.ho && ow < P.wo) ? (((img * P.ho + oh) * P.wo + ow) * kCo + 8 * cg) * 2 : (int)0x80000000;
      gv[u] = img_load16(rg, off);
      xv[u] = img_load16(rb, off);
    }
  };

  for (int i = tid; i < 6 * kCo; i += 256) cf[i] = P.coef[i];
  issue(t0, abuf0);
  fetch(t0);

  // per-lane bases of the transposed reads: pixel rows L and L + 16 of a K step
  const int g4 = lane >> 4, L = 4 * g4 + ((lane >> 2) & 3), p8 = (lane & 3) * 8;
  const int wm = wave / WN, wn = wave % WN;
  const int aoff = L * 16 + p8;
  const unsigned char* dbase[CB];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) dbase[cb] = dxs + L * 128 + (((wm * CB + cb) ^ ((L >> 1) & 3)) << 5) + p8;
  f32x4 acc[CB][NBW];
#pragma unroll
  for (int cb = 0; cb < CB; ++cb)
#pragma unroll
    for (int j = 0; j < NBW; ++j) acc[cb][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int act = ACT >= 0 ? ACT : P.act;

  // tile t, its image rows in buffer B (0 / 1: even / odd tiles of the run)
  auto tile = [&](int t, auto bc) {
    constexpr int B = decltype(bc)::value;
    int img, oh0, ow0;
    tile_xy(t, img, oh0, ow0);
    // tile t's g, x and image rows have landed (this wave's); every wave is done reading dx of
    // tile t - 1
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    {
      BnDx<8> k;
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const f32x4 va = *(const f32x4*)(cf + 8 * cg + 4 * q), vb = *(const f32x4*)(cf + kCo + 8 * cg + 4 * q);
        const f32x4 vk = *(const f32x4*)(cf + 2 * kCo + 8 * cg + 4 * q), vm = *(const f32x4*)(cf + 3 * kCo + 8 * cg + 4 * q);
        const f32x4 vs = *(const f32x4*)(cf + 4 * kCo + 8 * cg + 4 * q), vh = *(const f32x4*)(cf + 5 * kCo + 8 * cg + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          k.a[4 * q + e] = va[e]; k.b[4 * q + e] = vb[e]; k.k[4 * q + e] = vk[e];
          k.mu[4 * q + e] = vm[e]; k.sc[4 * q + e] = vs[e]; k.sh[4 * q + e] = vh[e];
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int px = pq + 32 * u;
        const bool ok = oh0 + (px >> 6) < P.ho && ow0 + (px & 63) < P.wo;
        const bf16x8 gb = __builtin_bit_cast(bf16x8, gv[u]), xb = __builtin_bit_cast(bf16x8, xv[u]);
        float gf[8], xf[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) { gf[j] = to_f(gb[j]); xf[j] = to_f(xb[j]); }
        bn_row_mask<bf16, 8>(gf, (const bf16*)nullptr, xf, k, act, 8);
        bf16x8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = ok ? from_f<bf16>(bn_bwd_dx<8>(k, j, gf[j], xf[j])) : (bf16)0.f;
        *(bf16x8*)(dxs + px * 128 + ((((cg >> 1) ^ ((px >> 1) & 3))) << 5) + (cg & 1) * 16) = o;
        __builtin_amdgcn_sched_barrier(0);  // pixel by pixel: one pixel's fp32 values live at a time
      }
    }
    __syncthreads();  // dx of tile t complete; all waves' image rows of tile t landed
    if (t + 1 < t1) {
      issue(t + 1, B ? abuf0 : abuf1);
      fetch(t + 1);
    }
    const unsigned char* ab = (B ? abuf1 : abuf0) + aoff;
#pragma unroll
    for (int kk = 0; kk < 2 * kTH; ++kk) {  // 32 pixels: tile row kk >> 1, columns 32 (kk & 1) ..
      bf16x8 fd[CB], fa[NBW];
#pragma unroll
      for (int cb = 0; cb < CB; ++cb) fd[cb] = img_tr_frag(dbase[cb] + 32 * kk * 128, dbase[cb] + (32 * kk + 16) * 128);
#pragma unroll
      for (int j = 0; j < NBW; ++j) {
        const int nb = wn * NBW + j, r = nb / NJ, jj = nb - r * NJ;
        const unsigned char* a0 = ab + ((2 * (kk >> 1) + r) * NC + 32 * (kk & 1) + 2 * jj) * 16;
        fa[j] = img_tr_frag(a0, a0 + 256);
      }
#pragma unroll
      for (int cb = 0; cb < CB; ++cb)
#pragma unroll
        for (int j = 0; j < NBW; ++j) acc[cb][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[j], fd[cb], acc[cb][j], 0, 0, 0);
    }
  };
  for (int t = t0; t < t1; t += 2) {
    tile(t, std::integral_constant<int, 0>());
    if (t + 1 < t1) tile(t + 1, std::integral_constant<int, 1>());
  }
  // acc[cb][j][e] = dW'[co = 16 (wm CB + cb) + (lane & 15)][row tap r][slot 2 jj + (g4 >> 1)][4 (g4 & 1) + e]:
  // tap s = 2 slot - 1 + (g4 & 1), channel e (e = 3: the padding channel)
  float* out = P.slab + (long)bid * W_EL;
#pragma unroll
  for (int cb = 0; cb < CB; ++cb) {
    const int co = 16 * (wm * CB + cb) + (lane & 15);
#pragma unroll
    for (int j = 0; j < NBW; ++j) {
      const int nb = wn * NBW + j, r = nb / NJ, jj = nb - r * NJ;
      const int s = 2 * (2 * jj + (g4 >> 1)) - 1 + (g4 & 1);
      if (s >= 0 && s < KW) {
        float* o = out + ((co * KH + r) * KW + s) * 3;
        o[0] = acc[cb][j][0];
        o[1] = acc[cb][j][1];
        o[2] = acc[cb][j][2];
      }
    }
  }
}

template <int ACT>
static const void* img_wg_kernel_act(int kh) {
  return kh == 7 ? (const void*)imgconv_bn_wgrad_kernel<7, 7, 2, ACT> : (const void*)imgconv_bn_wgrad_kernel<3, 3, 1, ACT>;
}
static const void* img_wg_kernel(int kh, int act) {
  const int v = img_act_variant(act);
  return v == 0 ? img_wg_kernel_act<0>(kh) : v == 1 ? img_wg_kernel_act<1>(kh) : img_wg_kernel_act<-1>(kh);
}
// Persistent grid as img_grid: one contiguous run of tiles per resident workgroup slot; every
// workgroup gets >= 1 tile and writes one slab.
static void img_wg_grid(const rtsds_conv_desc* d, int& grid, int& per) {
  static int occ[2] = {0, 0}, cus = 0;
  const int v = d->kh == 7;
  if (!occ[v] && (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ[v], img_wg_kernel(d->kh, RTSDS_ACT_RELU), 256, 0) != hipSuccess ||
                  occ[v] < 1))
    occ[v] = 1;
  if (!cus && (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus < 1)) cus = 256;
  const int tiles = img_tiles(d), slots = cus * occ[v];
  per = (tiles + slots - 1) / slots;
  grid = (tiles + per - 1) / per;
}
static bool img_wg_ok(const rtsds_conv_desc* d) { return check_desc(d) == RTSDS_OK && imgconv_ok(d); }
static size_t img_wg_slab_bytes(const rtsds_conv_desc* d) {
  int grid, per;
  img_wg_grid(d, grid, per);
  return al256((size_t)grid * d->k * d->kh * d->kw * 3 * 4);
}
extern "C" size_t rtsds_imgconv_bn_wgrad_workspace(const rtsds_conv_desc* d) {
  return img_wg_ok(d) ? img_wg_slab_bytes(d) + sp_x4_bytes(d) : 0;
}
static int img_wg_impl(const rtsds_conv_desc* d, const void* x, const void* bn_dy, const void* bn_x, const float* coef, int act,
                       float* dw, int accumulate, void* ws, size_t ws_bytes, rtsds_split_reduce_desc* pending, void* stream) {
  if (!img_wg_ok(d)) return check_desc(d) ? check_desc(d) : RTSDS_ERR_UNSUPPORTED;
  if (!(act == RTSDS_ACT_NONE || act == RTSDS_ACT_RELU || act == RTSDS_ACT_LEAKY)) return RTSDS_ERR_UNSUPPORTED;
  if (!x || !bn_dy || !bn_x || !coef || !dw) return RTSDS_ERR_SHAPE;
  const bool x_padded = (accumulate & RTSDS_INPUT_PADDED) != 0;
  accumulate &= ~RTSDS_INPUT_PADDED;
  if (ws_bytes < rtsds_imgconv_bn_wgrad_workspace(d)) return RTSDS_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t slab_bytes = img_wg_slab_bytes(d);
  if (!x_padded) {
    void* x4 = (char*)ws + slab_bytes;
    sp_pad4(d, x, x4, st);
    x = x4;
  }
  ImgWgArgs a;
  a.x4 = (const bf16*)x; a.g = (const bf16*)bn_dy; a.xb = (const bf16*)bn_x; a.coef = coef; a.slab = (float*)ws;
  a.n = d->n; a.h = d->h; a.w = d->w; a.ho = d->ho; a.wo = d->wo; a.ph = d->ph; a.pw = d->pw; a.act = act;
  a.tiles = img_tiles(d);
  int grid;
  img_wg_grid(d, grid, a.per);
  void* args[] = {&a};
  (void)hipLaunchKernel(img_wg_kernel(d->kh, act), dim3(grid), dim3(256), args, 0, st);
  // the slabs are already in dw's order: c = 4 "channels" per float4 output
  rtsds_split_reduce_desc q;
  q.slab = (const float*)ws;
  q.dw = dw;
  q.slab_stride = (long)d->k * d->kh * d->kw * 3;
  q.nv = d->k * d->kh * d->kw * 3 / 4;
  q.cv = 1;
  q.cp = 4;
  q.splits = grid;
  q.accumulate = accumulate ? 1 : 0;
  if (pending) {
    *pending = q;
    RET_LAUNCH();
  }
  return rtsds_split_reduce_many(1, &q, stream);
}
extern "C" int rtsds_imgconv_bn_wgrad(const rtsds_conv_desc* d, const void* x, const void* bn_dy, const void* bn_x,
                                      const float* coef, int act, float* dw, int accumulate, void* ws, size_t ws_bytes,
                                      void* stream) {
  return img_wg_impl(d, x, bn_dy, bn_x, coef, act, dw, accumulate, ws, ws_bytes, nullptr, stream);
}
extern "C" int rtsds_imgconv_bn_wgrad_deferred(const rtsds_conv_desc* d, const void* x, const void* bn_dy, const void* bn_x,
                                               const float* coef, int act, float* dw, int accumulate, void* ws,
                                               size_t ws_bytes, rtsds_split_reduce_desc* pending, void* stream) {
  if (!pending) return RTSDS_ERR_SHAPE;
  pending->nv = 0;
  return img_wg_impl(d, x, bn_dy, bn_x, coef, act, dw, accumulate, ws, ws_bytes, pending, stream);
}
