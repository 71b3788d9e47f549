// The arithmetic of one workgroup of the batched split-K reduction, shared by
// split_reduce_many_kernel (conv_wgrad.hip) and adam_slabs_kernel (optim.hip) so that the
// summation order cannot drift between the gradient the reduce writes and the one the fused
// optimizer step consumes.
#pragma once
#include "common.h"

// 256 threads = 64 float4 outputs x 4 split groups; output i of descriptor q (i >= q.nv: idle lane).
// Group sg sums splits sg, sg + 4, ... in ascending order with 8 loads in flight (clamped,
// unconditional; past-the-end ones contribute nothing); the four group sums are combined as
// (red0 + red1) + (red2 + red3).  Every thread of the workgroup must call it (one barrier); the
// sum is returned in t to the sg == 0 lanes with i < q.nv, t is unspecified elsewhere.
RT_DEV void split_reduce_block(const rtsds_split_reduce_desc& q, int i, float (*red)[64][4], float* t) {
  const int lane = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const bool ok = i < q.nv;
  const int rt = (ok ? i : 0) / q.cv;  // co * taps + tap
  const long src = (long)rt * q.cp + (long)((ok ? i : 0) - rt * q.cv) * 4;
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int g = sg; ok && g < q.splits; g += 32) {
    float v8[8][4];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const f32x4 v = *(const f32x4*)(q.slab + (long)min(g + 4 * u, q.splits - 1) * q.slab_stride + src);
#pragma unroll
      for (int e = 0; e < 4; ++e) v8[u][e] = v[e];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (g + 4 * u < q.splits)
#pragma unroll
        for (int e = 0; e < 4; ++e) s[e] += v8[u][e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[sg][lane][e] = s[e];
  __syncthreads();
  if (sg == 0 && ok) {
#pragma unroll
    for (int e = 0; e < 4; ++e) t[e] = (red[0][lane][e] + red[1][lane][e]) + (red[2][lane][e] + red[3][lane][e]);
  }
}
