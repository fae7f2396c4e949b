// The row distance of the descriptor searches (retrieval.hip: knn_dist_kernel; loop_closure.hip: knn_window_kernel), stated
// once so that both give the same bits: lane l of a wave sums elements l, l + 64, ... of the squared difference with fmaf, the
// 64 partial sums are folded by the xor butterfly 32 ... 1, and the root is sqrtf.  Exact difference form, as the reference.
#pragma once
#include "common.h"

namespace egonn {

// R rows, `row_stride` floats apart, against the query `s_q` (LDS): the R sums advance together so that their loads overlap;
// every sum sees the operations of R = 1 in the same order.  out[u]: the distance of row u, the same bits in every lane.
template <int R>
__device__ static inline void knn_row_distance(const float* __restrict__ row, int64_t row_stride, const float* s_q, int d, int lane,
                                               float (&out)[R]) {
  float s[R];
#pragma unroll
  for (int u = 0; u < R; ++u) s[u] = 0.f;
  for (int i = lane; i < d; i += 64) {
    const float qv = s_q[i];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const float df = row[u * row_stride + i] - qv;
      s[u] = fmaf(df, df, s[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < R; ++u) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s[u] += __shfl_xor(s[u], o, 64);
    out[u] = sqrtf(s[u]);
  }
}

}  // namespace egonn
