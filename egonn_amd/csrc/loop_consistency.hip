// Pairwise-consistency filter for loop edges ahead of the pose graph.
//
// Two loop closures taken close together in time must agree with each other through the odometry between them; a false one
// agrees with nobody.  Inputs: the drifting trajectory X (n,4,4) and loop edges e = (a, b, Z, w) with Z ~ X_a^-1 X_b, E rows, static.
// Live: the pose-graph plan would leave the edge on (pose_math.h: pose_edge_status), both its poses are finite (NONFINITE if
// not) and one of its two weights is positive.  A dead edge never votes, has support 0 and keep 0, and changes nothing else.
// Cycle of a pair of live edges:  C = Z_e (X_be^-1 X_bf) Z_f^-1 (X_af^-1 X_ae),  c_trans = |t_C|,  c_rot = |Log_SO3 R_C| with the
// logarithm of the pose graph.  C(e, f) and C(f, e) are conjugates: equal angles, different translation norms.  The relation
// is therefore made symmetric by construction: live edges are sorted by b (stable flat radix sort, dead edges behind with
// key n) and a pair is evaluated in one canonical role, the edge earlier in sorted order as e, by one function (lc_cycle) that
// is inlined once per kernel, so both edges of a pair see the same bit whichever wave evaluates it.
// Comparable: |b_e - b_f| <= window, |a_e - a_f| <= window, |pos_e - pos_f| <= H = max_partners / 2 in sorted positions.  A live
// edge with a partner inside its b-window beyond the position cap raises EGONN_LC_STATUS_TRUNCATED.
// Consistent: comparable, c_trans <= trans_thr + trans_drift g and c_rot <= rot_thr + rot_drift g, g = |b_e - b_f| + |a_e - a_f|.
// An edge never counts itself; two duplicates count each other.
// Selection: the min_support-core of the consistency graph in synchronous rounds: every survivor counts its surviving
// consistent partners, then all below min_support leave at once.  max_rounds rounds are enqueued; after a round that removed
// nothing the later ones return at once.  EGONN_LC_STATUS_ROUNDS when the last round still removed something.
//
// Kernel form.  lc_validate: one edge per lane, status and sort key.  lc_rows: one wave per sorted position s; lane l of
// chunk c takes partner position s - H + 64 c + l, evaluates the cycle in registers, and the wave's ballot is word c of the
// adjacency row of s (W = max_partners / 64 + 1 words, bit k = position s - H + k).  lc_round: one lane per position, one wave
// per word of the alive mask: popcount of row & alive window (the window taken from the position bitmask by a funnel
// shift); the mask is double-buffered, a round reads one and writes the other.  lc_finish: the final supports and outputs.
// Everything is float64 and integer, deterministic, on one stream, without host synchronisation, floating-point atomics, grid
// barriers or cooperative launches (the only atomics are integer ORs into status words).  The three round flags rotate:
// round r reads flag (r - 1) % 3, ORs into flag r % 3 and clears flag (r + 1) % 3, so no launch reads a word it may be writing.
#include "common.h"

#include <math.h>

#include "../../include/egonn_hip.h"
#include "pose_math.h"

namespace egonn {

static constexpr int LC_WG = 64;
static constexpr int LC_MAX_PARTNERS = 1 << 16;
static constexpr int LC_MAX_ROUNDS = 1 << 16;

struct LcState {
  int32_t flag[3], rounds;
};

// (c_trans, c_rot) of the cycle with (Ze, Xae, Xbe) in the role of e: every pointer is the start of a (4,4) row-major matrix
__device__ static inline void lc_cycle(const double* __restrict__ Ze, const double* __restrict__ Xae, const double* __restrict__ Xbe,
                                       const double* __restrict__ Zf, const double* __restrict__ Xaf, const double* __restrict__ Xbf,
                                       double* c_trans, double* c_rot) {
  double R0[9], t0[3], R1[9], t1[3], R2[9], t2[3];
  se3_load(Xbe, R0, t0);
  se3_load(Xbf, R1, t1);
  se3_inv_mul(R0, t0, R1, t1, R2, t2);                 // X_be^-1 X_bf
  se3_load(Ze, R0, t0);
  se3_mul(R0, t0, R2, t2, R1, t1);                     // Z_e (.)
  se3_load(Zf, R0, t0);
  se3_mul_inv(R1, t1, R0, t0, R2, t2);                 // (.) Z_f^-1
  se3_load(Xaf, R0, t0);
  se3_load(Xae, R1, t1);
  double R3[9], t3[3];
  se3_inv_mul(R0, t0, R1, t1, R3, t3);                 // X_af^-1 X_ae
  se3_mul(R2, t2, R3, t3, R0, t0);                     // C
  double ax[3], sn, cs;
  *c_rot = so3_log_angle(R0, ax, &sn, &cs);            // theta itself, the length of Log R: no theta / sin(theta), which is 0 * inf at a half turn
  *c_trans = sqrt(t0[0] * t0[0] + t0[1] * t0[1] + t0[2] * t0[2]);
}

// the filter's status of an edge: the plan's bits, NONFINITE also for a pose that is not finite
__device__ static inline int lc_edge_status(const double* __restrict__ X, int32_t n, int32_t a, int32_t b, const double* __restrict__ z,
                                            double wr, double wt) {
  int st = pose_edge_status(a, b, n, z, wr, wt);
  if (!(st & EGONN_PG_STATUS_BAD_INDEX) && !(pose_finite(X + (int64_t)a * 16) && pose_finite(X + (int64_t)b * 16)))
    st |= EGONN_PG_STATUS_NONFINITE;
  return st;
}

__global__ __launch_bounds__(LC_WG) void lc_validate_kernel(const double* __restrict__ X, int32_t n, const int32_t* __restrict__ edge_index,
                                                            const double* __restrict__ Z, const double* __restrict__ w, int32_t E,
                                                            int32_t* __restrict__ edge_status, uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals, LcState* __restrict__ st,
                                                            int32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * LC_WG + threadIdx.x;
  if (e == 0) st->flag[0] = 0, st->flag[1] = 0, st->flag[2] = 0, st->rounds = 0, *status = 0;
  if (e >= E) return;
  const int32_t a = edge_index[2 * e], b = edge_index[2 * e + 1];
  const double wr = w[2 * e], wt = w[2 * e + 1];
  const int s = lc_edge_status(X, n, a, b, Z + e * 16, wr, wt);
  const bool live = s == 0 && (wr > 0.0 || wt > 0.0);
  edge_status[e] = s;
  keys[e] = live ? (uint64_t)b : (uint64_t)n;                              // n: behind every live edge, as pg_csr_kernel has it
  vals[e] = (uint32_t)e;
}

// one wave per sorted position s: the adjacency row of s, support0 and the first alive mask
__global__ __launch_bounds__(LC_WG) void lc_rows_kernel(const double* __restrict__ X, int32_t n, const int32_t* __restrict__ edge_index,
                                                        const double* __restrict__ Z, int32_t E, const uint64_t* __restrict__ keys,
                                                        const uint32_t* __restrict__ vals, int32_t window, double trans_thr,
                                                        double rot_thr, double trans_drift, double rot_drift, int32_t H, int32_t W,
                                                        uint64_t* __restrict__ rows, uint64_t* __restrict__ alive,
                                                        int32_t* __restrict__ support0, int32_t* __restrict__ status) {
  const int64_t s = blockIdx.x;
  const int lane = threadIdx.x;
  if (s >= E) return;
  if (lane == 0 && (s & 63) == 0) {                                        // the alive word of positions s .. s + 63
    uint64_t word = 0;
    for (int k = 0; k < 64 && s + k < E; ++k)
      if (keys[s + k] != (uint64_t)n) word |= 1ull << k;
    alive[s >> 6] = word;
  }
  const uint64_t key = keys[s];
  const uint32_t me = vals[s];
  uint64_t* row = rows + s * W;
  if (key == (uint64_t)n) {                                                // dead: an empty row
    for (int c = lane; c < W; c += LC_WG) row[c] = 0;
    if (lane == 0) support0[me] = 0;
    return;
  }
  const int32_t bs = (int32_t)key, as = edge_index[2 * (int64_t)me];
  if (lane == 0) {                                                         // sorted by b: the next position past the cap decides
    const int64_t lo = s - H - 1, hi = s + H + 1;
    bool cut = lo >= 0 && (int64_t)bs - (int64_t)keys[lo] <= window;
    cut = cut || (hi < E && keys[hi] != (uint64_t)n && (int64_t)keys[hi] - (int64_t)bs <= window);
    if (cut) atomicOr(status, EGONN_LC_STATUS_TRUNCATED);
  }
  int count = 0;
  for (int c = 0; c < W; ++c) {
    const int64_t p = s - H + 64 * (int64_t)c + lane;
    bool ok = p >= 0 && p < E && p != s && p <= s + H;
    if (ok) {
      const uint64_t kp = keys[p];
      ok = kp != (uint64_t)n;
      if (ok) {
        const uint32_t other = vals[p];
        const int64_t ap = edge_index[2 * (int64_t)other], bp = (int64_t)kp;
        const int64_t db = bp > bs ? bp - bs : bs - bp, da = ap > as ? ap - as : as - ap;
        ok = db <= window && da <= window;
        if (ok) {
          const bool first = s < p;                                        // the earlier position plays e
          const int64_t ie = first ? me : other, jf = first ? other : me;
          const int64_t ae = first ? as : ap, be = first ? bs : bp, af = first ? ap : as, bf = first ? bp : bs;
          double ct, cr;
          lc_cycle(Z + ie * 16, X + ae * 16, X + be * 16, Z + jf * 16, X + af * 16, X + bf * 16, &ct, &cr);
          const double g = (double)(db + da);
          ok = ct <= trans_thr + trans_drift * g && cr <= rot_thr + rot_drift * g;        // false for NaN
        }
      }
    }
    const uint64_t word = __ballot(ok);
    if (lane == 0) row[c] = word;
    count += __popcll(word);
  }
  if (lane == 0) support0[me] = count;
}

// the alive bits of positions q .. q + 63 (q may be negative or reach past the end: those bits are 0)
__device__ static inline uint64_t lc_alive_window(const uint64_t* __restrict__ alive, int64_t nwords, int64_t q) {
  const int64_t wi = q >> 6;                                               // floor, also below 0
  const int sh = (int)(q & 63);
  const uint64_t lo = wi >= 0 && wi < nwords ? alive[wi] : 0, hi = wi + 1 >= 0 && wi + 1 < nwords ? alive[wi + 1] : 0;
  return sh ? (lo >> sh) | (hi << (64 - sh)) : lo;
}
__device__ static inline int lc_count(const uint64_t* __restrict__ rows, const uint64_t* __restrict__ alive, int64_t nwords, int64_t s,
                                      int32_t H, int32_t W) {
  int count = 0;
  for (int c = 0; c < W; ++c) count += __popcll(rows[s * W + c] & lc_alive_window(alive, nwords, s - H + 64 * (int64_t)c));
  return count;
}

// round r: one lane per position, one wave per alive word
__global__ __launch_bounds__(LC_WG) void lc_round_kernel(LcState* __restrict__ st, int r, int32_t E, int32_t H, int32_t W,
                                                         int32_t min_support, const uint64_t* __restrict__ rows,
                                                         const uint64_t* __restrict__ alive_in, uint64_t* __restrict__ alive_out) {
  const int prev = (r + 2) % 3, cur = r % 3, next = (r + 1) % 3;
  const bool stopped = r > 0 && st->flag[prev] == 0;                       // the round before removed nothing: a fixed point
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    st->flag[next] = 0;
    if (r > 0 && !stopped) st->rounds += 1;                                // written by this lane of every launch and by no other
  }
  if (stopped) return;                                                     // both masks are equal from here on
  const int64_t nwords = ((int64_t)E + 63) >> 6;
  const int64_t s = (int64_t)blockIdx.x * LC_WG + threadIdx.x;
  bool live = false, stay = false;
  if (s < E) {
    live = (alive_in[s >> 6] >> (s & 63)) & 1;
    stay = live && lc_count(rows, alive_in, nwords, s, H, W) >= min_support;
  }
  const uint64_t word = __ballot(stay), gone = __ballot(live && !stay);
  if (threadIdx.x == 0) {
    alive_out[blockIdx.x] = word;
    if (gone) atomicOr(&st->flag[cur], 1);
  }
}

__global__ __launch_bounds__(LC_WG) void lc_finish_kernel(const LcState* __restrict__ st, int max_rounds, int32_t E, int32_t H, int32_t W,
                                                          const uint64_t* __restrict__ rows, const uint64_t* __restrict__ alive,
                                                          const uint32_t* __restrict__ vals, const double* __restrict__ w,
                                                          uint8_t* __restrict__ keep, int32_t* __restrict__ support,
                                                          double* __restrict__ weights_out, int32_t* __restrict__ rounds,
                                                          int32_t* __restrict__ status) {
  const int64_t s = (int64_t)blockIdx.x * LC_WG + threadIdx.x;
  if (s == 0) {
    const int last = st->flag[(max_rounds - 1) % 3] != 0;                  // of the last round, if it ran
    *rounds = st->rounds + last;
    if (last) atomicOr(status, EGONN_LC_STATUS_ROUNDS);
  }
  if (s >= E) return;
  const int64_t nwords = ((int64_t)E + 63) >> 6;
  const bool live = (alive[s >> 6] >> (s & 63)) & 1;
  const int64_t e = vals[s];
  keep[e] = live;
  support[e] = live ? lc_count(rows, alive, nwords, s, H, W) : 0;
  weights_out[2 * e] = live ? w[2 * e] : 0.0, weights_out[2 * e + 1] = live ? w[2 * e + 1] : 0.0;
}

// the test seam of the arithmetic: one pair per lane, in the canonical role (the order of (b, row) is the sorted order)
__global__ __launch_bounds__(LC_WG) void lc_pairs_kernel(const double* __restrict__ X, int32_t n, const int32_t* __restrict__ edge_index,
                                                         const double* __restrict__ Z, int32_t E, const int32_t* __restrict__ pairs,
                                                         int64_t P, double* __restrict__ out) {
  const int64_t k = (int64_t)blockIdx.x * LC_WG + threadIdx.x;
  if (k >= P) return;
  const int64_t i = pairs[2 * k], j = pairs[2 * k + 1];
  double ct = NAN, cr = NAN;
  if (i >= 0 && i < E && j >= 0 && j < E) {
    const int32_t ai = edge_index[2 * i], bi = edge_index[2 * i + 1], aj = edge_index[2 * j], bj = edge_index[2 * j + 1];
    if (lc_edge_status(X, n, ai, bi, Z + i * 16, 1.0, 1.0) == 0 && lc_edge_status(X, n, aj, bj, Z + j * 16, 1.0, 1.0) == 0) {
      const bool first = bi < bj || (bi == bj && i <= j);
      const int64_t ie = first ? i : j, jf = first ? j : i;
      const int64_t ae = first ? ai : aj, be = first ? bi : bj, af = first ? aj : ai, bf = first ? bj : bi;
      lc_cycle(Z + ie * 16, X + ae * 16, X + be * 16, Z + jf * 16, X + af * 16, X + bf * 16, &ct, &cr);
    }
  }
  out[2 * k] = ct, out[2 * k + 1] = cr;
}

// ------------------------------------------------------------------ the scratch span
// With scratch = nullptr only `total` means anything
struct LcSpan {
  uint64_t* keys[2];        // ping-pong buffers of the sort
  uint32_t* vals[2];
  Arena sort_ws;
  uint64_t *rows, *alive[2];
  LcState* state;
  size_t total;
};
static bool lc_partners_ok(int max_partners) { return max_partners >= 64 && max_partners <= LC_MAX_PARTNERS && max_partners % 64 == 0; }
static LcSpan lc_span(void* scratch, int64_t E, int max_partners) {
  LcSpan S;
  Carve c(scratch);
  const size_t ee = (size_t)(E > 0 ? E : 1), W = (size_t)max_partners / 64 + 1, nwords = (ee + 63) / 64;
  for (int k = 0; k < 2; ++k) S.keys[k] = c.take<uint64_t>(ee);
  for (int k = 0; k < 2; ++k) S.vals[k] = c.take<uint32_t>(ee);
  S.sort_ws = c.sort_arena(radix_sort_scratch_bytes((int64_t)ee));
  S.rows = c.take<uint64_t>(ee * W);
  for (int k = 0; k < 2; ++k) S.alive[k] = c.take<uint64_t>(nwords);
  S.state = c.take<LcState>(1);
  S.total = c.total();
  return S;
}
static inline bool lc_thr_ok(double v) { return v >= 0.0 && v < INFINITY; }
static inline bool lc_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static inline unsigned lc_grid(int64_t items) { return (unsigned)cdiv(items > 0 ? items : 1, LC_WG); }

API int64_t egonn_loop_consistency_scratch_bytes(int64_t E, int max_partners) {
  if (!pose_sizes_ok(1, E) || !lc_partners_ok(max_partners)) return -1;
  return (int64_t)lc_span(nullptr, E, max_partners).total;
}

API int egonn_loop_consistency(const double* poses, int64_t n, const int32_t* edge_index, const double* Z, const double* weights,
                               int64_t E, int window, double trans_thr, double rot_thr, double trans_drift, double rot_drift,
                               int min_support, int max_rounds, int max_partners, uint8_t* keep, int32_t* support0, int32_t* support,
                               double* weights_out, int32_t* rounds, int32_t* edge_status, int32_t* status, void* scratch,
                               int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(pose_sizes_ok(n, E), EGONN_ERR_INVALID, "loop_consistency: n=%lld E=%lld outside 1 <= n < 2^31 - 1, 0 <= E < 2^30",
                (long long)n, (long long)E);
  EGONN_REQUIRE(poses && rounds && status && (E == 0 || (edge_index && Z && weights && keep && support0 && support && weights_out &&
                                                         edge_status)),
                EGONN_ERR_INVALID, "loop_consistency: null pointer");
  EGONN_REQUIRE(lc_aligned(poses, 8) && lc_aligned(Z, 8) && lc_aligned(weights, 8) && lc_aligned(weights_out, 8) &&
                    lc_aligned(edge_index, 4) && lc_aligned(support0, 4) && lc_aligned(support, 4) && lc_aligned(rounds, 4) &&
                    lc_aligned(edge_status, 4) && lc_aligned(status, 4),
                EGONN_ERR_INVALID, "loop_consistency: a pointer is misaligned (8 bytes for float64, 4 for int32)");
  EGONN_REQUIRE(window >= 0, EGONN_ERR_INVALID, "loop_consistency: window=%d is negative", window);
  EGONN_REQUIRE(lc_thr_ok(trans_thr) && lc_thr_ok(rot_thr) && lc_thr_ok(trans_drift) && lc_thr_ok(rot_drift), EGONN_ERR_INVALID,
                "loop_consistency: a threshold is negative or not finite (trans_thr=%g rot_thr=%g trans_drift=%g rot_drift=%g)",
                trans_thr, rot_thr, trans_drift, rot_drift);
  EGONN_REQUIRE(min_support >= 1, EGONN_ERR_INVALID, "loop_consistency: min_support=%d must be positive", min_support);
  EGONN_REQUIRE(max_rounds >= 1 && max_rounds <= LC_MAX_ROUNDS, EGONN_ERR_INVALID, "loop_consistency: max_rounds=%d outside [1, %d]",
                max_rounds, LC_MAX_ROUNDS);
  EGONN_REQUIRE(lc_partners_ok(max_partners), EGONN_ERR_INVALID,
                "loop_consistency: max_partners=%d is not a positive multiple of 64 (up to %d)", max_partners, LC_MAX_PARTNERS);
  LcSpan S = lc_span(scratch, E, max_partners);
  EGONN_TRY(span_check("loop_consistency", scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  uint64_t *keys0 = S.keys[0], *keys1 = S.keys[1], *kres = keys1;
  uint32_t *vals0 = S.vals[0], *vals1 = S.vals[1], *vres = vals1;
  uint64_t *rows = S.rows, *const* alive = S.alive;
  LcState* state = S.state;
  const int32_t nn = (int32_t)n, ee = (int32_t)E, H = max_partners / 2, W = max_partners / 64 + 1;
  hipLaunchKernelGGL(lc_validate_kernel, dim3(lc_grid(E)), dim3(LC_WG), 0, st, poses, nn, edge_index, Z, weights, ee, edge_status, keys0,
                     vals0, state, status);
  if (E > 0) {
    int nbits = 1;
    while ((n >> nbits) != 0) ++nbits;                       // keys are 0 .. n
    EGONN_TRY(radix_sort_pairs(S.sort_ws, keys0, vals0, keys1, vals1, E, nbits, st, nullptr, &kres, &vres));
    hipLaunchKernelGGL(lc_rows_kernel, dim3((unsigned)E), dim3(LC_WG), 0, st, poses, nn, edge_index, Z, ee, kres, vres, (int32_t)window,
                       trans_thr, rot_thr, trans_drift, rot_drift, H, W, rows, alive[0], support0, status);
    for (int r = 0; r < max_rounds; ++r)
      hipLaunchKernelGGL(lc_round_kernel, dim3(lc_grid(E)), dim3(LC_WG), 0, st, state, r, ee, H, W, (int32_t)min_support, rows,
                         alive[r & 1], alive[(r + 1) & 1]);
  }
  hipLaunchKernelGGL(lc_finish_kernel, dim3(lc_grid(E)), dim3(LC_WG), 0, st, state, E > 0 ? max_rounds : 1, ee, H, W, rows,
                     alive[max_rounds & 1], vres, weights, keep, support, weights_out, rounds, status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_loop_cycle_errors(const double* poses, int64_t n, const int32_t* edge_index, const double* Z, int64_t E,
                                const int32_t* pairs, int64_t P, double* out, void* stream) {
  EGONN_REQUIRE(pose_sizes_ok(n, E) && P >= 0 && P < (1ll << 30), EGONN_ERR_INVALID,
                "loop_cycle_errors: n=%lld E=%lld P=%lld outside 1 <= n < 2^31 - 1, 0 <= E < 2^30, 0 <= P < 2^30", (long long)n,
                (long long)E, (long long)P);
  EGONN_REQUIRE(poses && (E == 0 || (edge_index && Z)) && (P == 0 || (pairs && out)), EGONN_ERR_INVALID,
                "loop_cycle_errors: null pointer");
  EGONN_REQUIRE(lc_aligned(poses, 8) && lc_aligned(Z, 8) && lc_aligned(out, 8) && lc_aligned(edge_index, 4) && lc_aligned(pairs, 4),
                EGONN_ERR_INVALID, "loop_cycle_errors: a pointer is misaligned (8 bytes for float64, 4 for int32)");
  if (P == 0) return EGONN_OK;
  hipLaunchKernelGGL(lc_pairs_kernel, dim3(lc_grid(P)), dim3(LC_WG), 0, (hipStream_t)stream, poses, (int32_t)n, edge_index, Z, (int32_t)E,
                     pairs, P, out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
