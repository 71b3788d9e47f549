// Helpers shared by the memory-bound translation units (layout.hip, pool.hip, chan.hip,
// resize.hip, optim.hip): launch sizing, grid-stride loops and the LDS staging of per-pixel
// channel rows.  All activations are NHWC; per-pixel channel vectors are contiguous.
#pragma once
#include "common.h"
#include <algorithm>
#include <climits>
#include <cmath>

static inline int ew_blocks(long work, int per_block = 256, int cap = 8192) {
  return (int)std::max<long>(1, std::min<long>(cap, (work + per_block - 1) / per_block));
}
#define GRID_STRIDE(i, n) for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)
// XCD-aware variant: workgroups b and b + 8 run on one XCD, so logical block = the XCD's
// contiguous run (bijective) -- neighbouring output rows (which share input rows) stay in one
// XCD's L2.
RT_DEV long xcd_block() {
  const int nwg = gridDim.x, b = blockIdx.x, xcd = b & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
}
#define GRID_STRIDE_XCD(i, n) for (long i = xcd_block() * (long)blockDim.x + threadIdx.x; i < (n); i += (long)gridDim.x * blockDim.x)

// ------------------------------------------------------------------ LDS-staged per-pixel kernels
// The per-pixel channel loops (C = 19 classes) read/write rows of C*sizeof(T) bytes (38 B for
// bf16) that are not 16-B aligned per pixel.  These variants move a block's 256 pixels
// (256*C elements, contiguous in NHWC) between HBM and LDS with 16-B vector accesses and
// run the per-pixel math out of LDS, so global traffic is fully coalesced.
static const int kStagePix = 256;
template <typename T>
RT_DEV void stage_in(const T* __restrict__ g, T* s, int nel) {
  const int nb = nel * (int)sizeof(T);
  const char* gb = (const char*)g;
  char* sb = (char*)s;
  if ((((uintptr_t)gb) & 15) == 0) {
    const int nv = nb >> 4;
    for (int i = threadIdx.x; i < nv; i += blockDim.x) ((uint4*)sb)[i] = ((const uint4*)gb)[i];
    for (int i = (nv << 4) / (int)sizeof(T) + threadIdx.x; i < nel; i += blockDim.x) s[i] = g[i];
  } else {
    for (int i = threadIdx.x; i < nel; i += blockDim.x) s[i] = g[i];
  }
}
template <typename T>
RT_DEV void stage_out(T* __restrict__ g, const T* s, int nel) {
  const int nb = nel * (int)sizeof(T);
  char* gb = (char*)g;
  const char* sb = (const char*)s;
  if ((((uintptr_t)gb) & 15) == 0) {
    const int nv = nb >> 4;
    for (int i = threadIdx.x; i < nv; i += blockDim.x) ((uint4*)gb)[i] = ((const uint4*)sb)[i];
    for (int i = (nv << 4) / (int)sizeof(T) + threadIdx.x; i < nel; i += blockDim.x) g[i] = s[i];
  } else {
    for (int i = threadIdx.x; i < nel; i += blockDim.x) g[i] = s[i];
  }
}
// The tile loop of a staged kernel: STAGE_TILES(p0, total) { np = tile_in(..); per-pixel work under
// threadIdx.x < np; tile_out(..) where the tile is an output }.  tile_in stages the tile's rows of
// every input (the i-th into the i-th [kStagePix][c] buffer) between two barriers, tile_out stores
// the first buffer behind one: every thread of the block must reach each call.
template <typename T>
RT_DEV T* stage_buf() {  // the kernel's dynamic LDS
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  return (T*)smem_raw;
}
#define STAGE_TILES(p0, total) for (long p0 = (long)blockIdx.x * kStagePix; p0 < (total); p0 += (long)gridDim.x * kStagePix)
template <typename T, typename... X>
RT_DEV int tile_in(T* buf, long p0, long total, int c, const X*... x) {
  const int np = (int)min<long>(kStagePix, total - p0);
  __syncthreads();
  ((stage_in(x + p0 * c, buf, np * c), buf += kStagePix * c), ...);  // one buffer per input, in order
  __syncthreads();
  return np;
}
template <typename T>
RT_DEV void tile_out(T* __restrict__ y, const T* buf, long p0, int np, int c) {
  __syncthreads();
  stage_out(y + p0 * c, buf, np * c);
}
