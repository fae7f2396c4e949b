// The batched iterate-until-stopped loop shared by the ICP (icp.hip, both estimators) and the NDT registration (ndt.hip); the
// normals' kNN pass of icp.hip uses its indexing.  P pairs share one flat grid: pair p owns the workgroups [wg0[p], wg0[p + 1]),
// one per PAIR_WG consecutive source points counted from the pair's own first point.  A round is two launches:
//
//   evaluate   every lane puts its point's terms into v[NP]; pair_reduce leaves the workgroup's sums in partial[flat * NP + k].
//   finish     one wave per pair: pair_gather sums the pair's partials in ascending workgroup order into s[NP]; the caller
//              writes its two metrics and decides; then pair_stop, or a step (U, ut) into pair_advance.
//
// That a pair has the same bits alone, in any batch and at any batch position rests on exactly these lines: the partition
// (pair_begin, pair_of, pair_chunk), the tree (pair_reduce) and the ascending gather (pair_gather).  A new estimator supplies
// the per-lane terms, a stop rule and a step.  Contraction is off; of pose_math.h only the loads and stores are used.  The
// search and kNN kernels of icp.hip spell the early-out and R s + t out themselves: with pair_chunk / pair_apply, or the state
// below as a base struct, they compile to other register assignments and measured up to 5 % slower.
#pragma once

#include "../../include/egonn_hip.h"
#include "common.h"
#include "pose_math.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int PAIR_WG = 256;               // lanes of an evaluating workgroup = source points per workgroup
static_assert(PAIR_WG == 4 * 64, "pair_reduce adds the sums of exactly four waves");

// The per-pair state: members of the estimator's own pair struct (`Pair` below), which keeps its layout.  double R[9], t[3]
// (T_k); int64_t so (first source point); int32_t ns, done, status.

// ------------------------------------------------------------------ pose plumbing
// o = R s + t, every row as ((R0 x + R1 y) + R2 z) + t
template <class Pair>
__device__ static inline void pair_apply(const Pair* __restrict__ q, const double* __restrict__ s, double* o) {
  const double x = s[0], y = s[1], z = s[2];
#pragma unroll
  for (int a = 0; a < 3; ++a) o[a] = ((q->R[a * 3] * x + q->R[a * 3 + 1] * y) + q->R[a * 3 + 2] * z) + q->t[a];
}

// ------------------------------------------------------------------ the flat grid
// Pair p before round 0: its source range (offsets clipped to ns_cap), T_0, row 0 of its T_trace rows, and its first workgroup,
// a function of the sizes of the pairs before it only.  The last pair closes the table with wg0[P].
template <class Pair>
__device__ static inline void pair_begin(Pair* q, const int64_t* __restrict__ soff, int64_t ns_cap, int P, int p,
                                         const double* __restrict__ T_init, double* __restrict__ T_trace, int max_it,
                                         int32_t* __restrict__ wg0) {
  const int64_t so = clipi(soff[p], ns_cap), se = clipi(soff[p + 1], ns_cap);
  const int64_t ns = se > so ? se - so : 0;
  if (T_init) se3_load(T_init + (size_t)p * 16, q->R, q->t);      // T_0: row p of a (P, 4, 4) T_init, the identity without one
  else for (int k = 0; k < 9; ++k) q->R[k] = k % 4 == 0 ? 1.0 : 0.0, q->t[k / 3] = 0.0;
  q->so = so, q->ns = (int32_t)ns, q->done = 0, q->status = 0;
  if (T_trace) se3_store(q->R, q->t, T_trace + ((size_t)p * (max_it + 1)) * 16);
  int64_t w = 0;
  for (int b = 0; b < p; ++b) {
    const int64_t a = clipi(soff[b], ns_cap), e = clipi(soff[b + 1], ns_cap);
    w += e > a ? (e - a + PAIR_WG - 1) / PAIR_WG : 0;
  }
  wg0[p] = (int32_t)w;
  if (p == P - 1) wg0[P] = (int32_t)(w + (ns + PAIR_WG - 1) / PAIR_WG);
}

// pair of workgroup `flat`: the largest p with wg0[p] <= flat
__device__ static inline int pair_of(const int32_t* __restrict__ wg0, int P, int flat) {
  int lo = 0, hi = P - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (wg0[mid] <= flat) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// which PAIR_WG source points of pair q (first workgroup `first`) workgroup `flat` owns; -1: none, the pair has stopped or the
// workgroup is slack of the grid's rounding.  Workgroup-uniform.
template <class Pair>
__device__ static inline int pair_chunk(const Pair* __restrict__ q, int first, int flat) {
  const int chunk = flat - first;
  return (q->done || chunk < 0 || (int64_t)chunk * PAIR_WG >= q->ns) ? -1 : chunk;
}

// the workgroup's sums of every lane's v[NP] into partial[flat * NP + k]: xor-shuffle tree per wave, then ((w0 + w1) + w2) + w3
// through s_red, NP x 4 doubles of LDS that the kernel declares
template <int NP>
__device__ __forceinline__ void pair_reduce(double* v, double (*s_red)[4], double* __restrict__ partial, int flat, int lane, int w) {
  const int t = threadIdx.x;
#pragma unroll
  for (int k = 0; k < NP; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);      // a fixed tree
    if (lane == 0) s_red[k][w] = v[k];
  }
  __syncthreads();
  if (t < NP) partial[(size_t)flat * NP + t] = ((s_red[t][0] + s_red[t][1]) + s_red[t][2]) + s_red[t][3];
}

// finish kernel, NP <= 64 lanes: the partials of pair q in ascending workgroup order into s[NP] (LDS); ends in a barrier
template <int NP, class Pair>
__device__ __forceinline__ void pair_gather(const Pair* __restrict__ q, int first, const double* __restrict__ partial, double* s) {
  const int t = threadIdx.x, nwg = (q->ns + PAIR_WG - 1) / PAIR_WG;
  if (t < NP) {
    double acc = 0.0;
    for (int c = 0; c < nwg; ++c) acc += partial[(size_t)(first + c) * NP + t];     // ascending workgroups
    s[t] = acc;
  }
  __syncthreads();
}

// ------------------------------------------------------------------ stop and advance
// pair p ends at `round` with status st under its T_k; the caller writes its two metrics
template <class Pair>
__device__ static inline void pair_stop(Pair* q, int p, int round, int st, double* __restrict__ T_out,
                                        int32_t* __restrict__ iterations, int32_t* __restrict__ status) {
  se3_store(q->R, q->t, T_out + (size_t)p * 16);
  iterations[p] = round, status[p] = st;
  q->status = st, q->done = 1;
}

// T_k+1 = U T_k and row round + 1 of the pair's T_trace rows
template <class Pair>
__device__ static inline void pair_advance(Pair* q, int p, int round, int max_it, const double* U, const double* ut,
                                           double* __restrict__ T_trace) {
  double Rn[9], tn[3];
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) Rn[r * 3 + c] = U[r * 3] * q->R[c] + U[r * 3 + 1] * q->R[3 + c] + U[r * 3 + 2] * q->R[6 + c];
    tn[r] = U[r * 3] * q->t[0] + U[r * 3 + 1] * q->t[1] + U[r * 3 + 2] * q->t[2] + ut[r];
  }
  for (int k = 0; k < 9; ++k) q->R[k] = Rn[k];
  for (int k = 0; k < 3; ++k) q->t[k] = tn[k];
  if (T_trace) se3_store(Rn, tn, T_trace + ((size_t)p * (max_it + 1) + round + 1) * 16);
}

// ------------------------------------------------------------------ host side
struct PairLayout {         // the caller carves its partial sums, n_wg * NP doubles, where it wants them
  void* pairs;              // n_pairs of the estimator's pair struct
  int32_t* wg0;
  int64_t n_wg;             // workgroups of the flat grid: every pair rounds its own up
};
static inline PairLayout pair_layout(Carve& c, int64_t n_src, int n_pairs, size_t pair_bytes) {
  PairLayout L;
  L.n_wg = cdiv(n_src, PAIR_WG) + n_pairs;
  L.pairs = c.take<char>((size_t)n_pairs * pair_bytes);
  L.wg0 = c.take<int32_t>((size_t)n_pairs + 1);
  return L;
}

// rows beyond a pair's last round read zero: (P, max_iteration + 1, 4, 4) T_trace, (P, max_iteration + 1, eval_width) eval_trace
static inline int pair_clear_traces(double* T_trace, double* eval_trace, int eval_width, int n_pairs, int max_iteration, hipStream_t st) {
  const size_t rows = (size_t)n_pairs * ((size_t)max_iteration + 1);
  if (T_trace) HIP_CHECK(hipMemsetAsync(T_trace, 0, rows * 16 * sizeof(double), st));
  if (eval_trace) HIP_CHECK(hipMemsetAsync(eval_trace, 0, rows * eval_width * sizeof(double), st));
  return EGONN_OK;
}

}  // namespace egonn
