// Pose-graph optimisation over odometry and loop edges: the corrected trajectory behind the loop detector.
//
// Problem.  Unknowns are poses X_i = [R_i | t_i], i < n, float64, (n,4,4) row-major.  Edge e = (a, b, Z, w) measures
// Z ~ X_a^-1 X_b with two weights w = (w_rot, w_trans) >= 0 in 1/sigma^2; both 0 switches the edge off.
//   M = X_a^-1 X_b,  E = Z^-1 M,  r = [t_E ; Log_SO3(R_E)] in R^6,  s = sqrt(w_trans |t_E|^2 + w_rot |Log R_E|^2),
//   rho_e = 1, or with robust_delta > 0 the IRLS weight of a Huber kernel, min(1, delta / s_e), recomputed at every
//   linearisation and held fixed inside the linear solve;  cost = sum_e rho_e (1 - rho_e / 2) s_e^2: s^2 / 2 for rho = 1 and
//   delta s - delta^2 / 2 beyond delta, the Huber cost, whose gradient is sum J^T rho W r (the solver's right-hand side), so that a
//   damped Gauss-Newton step is a descent step of the very number the accept test compares.
// Retraction: R_i <- R_i Exp(w_i), t_i <- t_i + R_i v_i with delta_i = (v_i, w_i); the product R Exp(w) is followed by one
// Newton-Schulz step R <- R (3 I - R^T R) / 2, which squares the distance to the orthogonal group (1e-15 stays 1e-15 over any
// number of updates).  A node whose delta is exactly zero is copied, not multiplied: fixed nodes (the gauge: a mask, default
// node 0) and nodes without a live edge come out bit-unchanged.
// Jacobians for this retraction (T = [t_M]x, R_Z^T = R_E R_M^T, Jri = the inverse right Jacobian of SO(3) at Log R_E):
//   side b:  d t_E = R_E v_b                    d phi = Jri w_b
//   side a:  d t_E = R_Z^T (-v_a + T w_a)       d phi = -Jri R_M^T w_a
// Kernel form: the linearisation stores R_E, Jri, R_M, t_M, the two effective weights and the residual (38 doubles per edge,
// padded to 40) and the two 6x6 blocks are applied analytically; two dense blocks would be 72 doubles and buy nothing.
// Logarithm: theta = atan2(|axial vector|, (trace - 1) / 2), exact in both tails.  theta / sin(theta) and the coefficient of
// [phi]x^2 in Jri, 1/theta^2 - (1 + cos) / (2 theta sin), switch to their Taylor series below theta = 0.05: the closed form of
// the coefficient cancels to a relative error of 2^-53 / theta^2 (4e-14 at 0.05), the series truncated after theta^4 is off by
// theta^6 / 1209600 (1.3e-14 at 0.05), so both are below 1e-13 on their side.  Residual rotations up to pi - 1e-3 are supported;
// beyond that the axial vector loses its direction, the edge gets EGONN_PG_STATUS_ANGLE and weight 0 for that linearisation.
//
// Everything is float64, on one stream, without host synchronisation, floating-point atomics, grid barriers or cooperative
// launches.  One node (or edge) per lane, 64 lanes per workgroup.  A reduction over the graph is two-stage: every workgroup
// writes one partial, every consumer re-sums all partials in one fixed order (lane-strided, then a butterfly).
// pg_odometry                   edges i -> i + 1 with Z = X_i^-1 X_{i+1} from a trajectory
// pg_validate / sort / pg_csr   the plan: edge status, node -> (edge, side) lists in edge order (the stable flat radix sort)
// pg_linearize                  per edge: residual, rho, the edge record, the cost term
// pg_setup                      per node: gradient, the 6x6 diagonal block + lambda I factored LDL^T, PCG start
// pg_pcg_a / pg_pcg_b           one PCG iteration in two launches: a = p update folded into H p (p double-buffered), b = x, r, z
// pg_retract, pg_node_cost, pg_decide   candidate poses, their cost, accept / reject / stop in a state struct on the device
// The two flags of the PCG are written by one kernel and read by the other, never both in one launch, so no launch reads a
// word it may be writing: a stopped solve makes every later launch return at once.
#include "common.h"

#include <math.h>

#include "../../include/egonn_hip.h"
#include "pose_math.h"

namespace egonn {

static constexpr int PG_WG = 64;
static constexpr int PG_LIN = 40;                    // doubles per linearised edge: 32 + the residual (6), padded to 64 bytes
static constexpr double PG_SMALL = POSE_LOG_SMALL;   // series below this angle (see above)
static constexpr double PG_MAX_ANGLE = 3.14159265358979323846 - 1e-3;

struct PgState {
  double lambda, cost;
  int32_t cur, done, iter, accepted, flag_a, flag_b;
};

__device__ static inline double pg_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ static inline double pg_wave_max(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// the sum of m partials, the same bits in every lane of every workgroup
__device__ static inline double pg_sum(const double* __restrict__ p, int m) {
  double acc = 0.0;
  for (int j = threadIdx.x; j < m; j += PG_WG) acc += p[j];
  return pg_wave_sum(acc);
}

// ------------------------------------------------------------------ plan
__global__ __launch_bounds__(PG_WG) void pg_validate_kernel(const int32_t* __restrict__ edge_index, const double* __restrict__ Z,
                                                            const double* __restrict__ w, int32_t n, int32_t E, int32_t* __restrict__ ab,
                                                            double* __restrict__ weff, int32_t* __restrict__ pstat,
                                                            int32_t* __restrict__ edge_status, uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals) {
  const int64_t e = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  if (e >= E) return;
  const int32_t a = edge_index[2 * e], b = edge_index[2 * e + 1];
  const double wr = w ? w[2 * e] : 1.0, wt = w ? w[2 * e + 1] : 1.0;
  const int st = pose_edge_status(a, b, n, Z + e * 16, wr, wt);
  const bool live = st == 0 && (wr > 0.0 || wt > 0.0);
  ab[2 * e] = live ? a : 0, ab[2 * e + 1] = live ? b : 0;
  weff[2 * e] = live ? wr : 0.0, weff[2 * e + 1] = live ? wt : 0.0;
  pstat[e] = st;
  edge_status[e] = st;
  keys[2 * e] = live ? (uint64_t)a : (uint64_t)n, keys[2 * e + 1] = live ? (uint64_t)b : (uint64_t)n;    // n: behind every node
  vals[2 * e] = (uint32_t)(2 * e), vals[2 * e + 1] = (uint32_t)(2 * e + 1);
}

__device__ static inline int32_t pg_lower_bound(const uint64_t* __restrict__ keys, int32_t m, uint64_t x) {
  int32_t a = 0, b = m;
  while (a < b) {
    const int32_t mid = a + ((b - a) >> 1);
    if (keys[mid] < x) a = mid + 1; else b = mid;
  }
  return a;
}

// keys / vals: the sorted (node, 2 edge + side) pairs (null with no edge).  row_start (n + 1), inc (m), fixed resolved
__global__ __launch_bounds__(PG_WG) void pg_csr_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals, int32_t m,
                                                       int32_t n, const uint8_t* __restrict__ fixed_in, int32_t* __restrict__ row_start,
                                                       uint32_t* __restrict__ inc, uint8_t* __restrict__ fixed,
                                                       int32_t* __restrict__ graph_status) {
  const int64_t i = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  if (i < m) inc[i] = vals[i];
  if (i > n) return;
  const int32_t lo = m ? pg_lower_bound(keys, m, (uint64_t)i) : 0;
  row_start[i] = lo;
  if (i == n) return;
  const int32_t hi = m ? pg_lower_bound(keys, m, (uint64_t)i + 1) : 0;
  const uint8_t f = fixed_in ? (fixed_in[i] != 0) : (i == 0);
  fixed[i] = f;
  if (!f && hi == lo) atomicOr(graph_status, EGONN_PG_STATUS_ISOLATED);
}

// odometry edges of a trajectory: edge i = (i, i + 1), Z_i = X_i^-1 X_{i+1}, the difference of the translations taken first
__global__ __launch_bounds__(PG_WG) void pg_odometry_kernel(const double* __restrict__ X, int32_t m, double* __restrict__ Z,
                                                            int32_t* __restrict__ edge_index) {
  const int64_t i = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  if (i >= m) return;
  const double* Xa = X + i * 16;
  const double* Xb = Xa + 16;
  double Ra[9], ta[3], Rb[9], tb[3], RM[9], tM[3];
  se3_load(Xa, Ra, ta);
  se3_load(Xb, Rb, tb);
  se3_inv_mul(Ra, ta, Rb, tb, RM, tM);
  double* z = Z + i * 16;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) z[4 * a + b] = RM[3 * a + b];
    z[4 * a + 3] = tM[a];
  }
  z[12] = z[13] = z[14] = 0.0, z[15] = 1.0;
  edge_index[2 * i] = (int32_t)i, edge_index[2 * i + 1] = (int32_t)i + 1;
}

// ------------------------------------------------------------------ state
__global__ __launch_bounds__(PG_WG) void pg_init_kernel(PgState* __restrict__ st, double lambda, double* __restrict__ cost_trace,
                                                        int32_t* __restrict__ accept_trace, int max_it) {
  const int t = threadIdx.x;
  if (t == 0) {
    st->lambda = lambda, st->cost = 0.0;
    st->cur = 0, st->done = 0, st->iter = 0, st->accepted = 0, st->flag_a = 0, st->flag_b = 0;
  }
  if (cost_trace)
    for (int j = t; j <= max_it; j += PG_WG) cost_trace[j] = NAN;
  if (accept_trace)
    for (int j = t; j < max_it; j += PG_WG) accept_trace[j] = -1;
}

// ------------------------------------------------------------------ linearise: one edge per lane
// which: 0 = the current poses, 1 = the candidate.  first: edge_status starts from the plan's bits.
__global__ __launch_bounds__(PG_WG) void pg_linearize_kernel(const PgState* __restrict__ st, const double* __restrict__ X0,
                                                             const double* __restrict__ X1, int which, int first, int32_t E,
                                                             const int32_t* __restrict__ ab, const double* __restrict__ weff,
                                                             const int32_t* __restrict__ pstat, const double* __restrict__ Z,
                                                             double delta, double* __restrict__ lin0, double* __restrict__ lin1,
                                                             double* __restrict__ resid, double* __restrict__ ecost,
                                                             double* __restrict__ rho_out, double* __restrict__ s_out,
                                                             int32_t* __restrict__ edge_status) {
  if (st->done) return;
  const int64_t e = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  if (e >= E) return;
  const int sel = st->cur ^ which;
  const double* X = sel ? X1 : X0;
  double* L = (sel ? lin1 : lin0) + e * PG_LIN;
  double wr = weff[2 * e], wt = weff[2 * e + 1];
  int status = first ? pstat[e] : edge_status[e];
  double r[6] = {0, 0, 0, 0, 0, 0}, s = 0.0, rho = 1.0;
  if (wr > 0.0 || wt > 0.0) {                                              // a live edge of the plan
    const double* Xa = X + (int64_t)ab[2 * e] * 16;
    const double* Xb = X + (int64_t)ab[2 * e + 1] * 16;
    const double* z = Z + e * 16;
    double Ra[9], ta[3], Rb[9], tb[3], RZ[9], tZ[3], RM[9], tM[3], RE[9];
    se3_load(Xa, Ra, ta);
    se3_load(Xb, Rb, tb);
    se3_load(z, RZ, tZ);
    se3_inv_mul(Ra, ta, Rb, tb, RM, tM);                                   // M = X_a^-1 X_b: the difference first, so UTM-scale offsets cancel exactly
    se3_inv_mul(RZ, tZ, RM, tM, RE, r);                                    // E = Z^-1 M
    double ax[3], sn, cs;
    const double th = so3_log_angle(RE, ax, &sn, &cs), th2 = th * th;
    double k, c;
    if (th < PG_SMALL) {
      k = so3_log_series(th2);
      c = 1.0 / 12.0 + th2 * (1.0 / 720.0 + th2 * (1.0 / 30240.0));
    } else {
      k = th / sn;
      c = 1.0 / th2 - (1.0 + cs) / (2.0 * th * sn);
    }
    // past the range, or a residual that is not finite (a non-finite pose): NaN fails both comparisons
    const bool off = !(th <= PG_MAX_ANGLE) || !(fabs(r[0]) + fabs(r[1]) + fabs(r[2]) < INFINITY);
    if (off) {                                                             // weight 0, residual 0 and a record that holds no NaN
      status |= EGONN_PG_STATUS_ANGLE;
      wr = wt = 0.0;
      k = c = 0.0;
      r[0] = r[1] = r[2] = 0.0;
#pragma unroll
      for (int j = 0; j < 9; ++j) RE[j] = RM[j] = (j % 4 == 0) ? 1.0 : 0.0;
      tM[0] = tM[1] = tM[2] = 0.0;
    }
    const double p0 = off ? 0.0 : ax[0] * k, p1 = off ? 0.0 : ax[1] * k, p2 = off ? 0.0 : ax[2] * k, pp = p0 * p0 + p1 * p1 + p2 * p2;
    r[3] = p0, r[4] = p1, r[5] = p2;
    // Jri = I + [phi]x / 2 + c [phi]x^2,  [phi]x^2 = phi phi^T - |phi|^2 I
    double J[9];
    J[0] = 1.0 + c * (p0 * p0 - pp), J[1] = -0.5 * p2 + c * p0 * p1, J[2] = 0.5 * p1 + c * p0 * p2;
    J[3] = 0.5 * p2 + c * p0 * p1, J[4] = 1.0 + c * (p1 * p1 - pp), J[5] = -0.5 * p0 + c * p1 * p2;
    J[6] = -0.5 * p1 + c * p0 * p2, J[7] = 0.5 * p0 + c * p1 * p2, J[8] = 1.0 + c * (p2 * p2 - pp);
    const double s2 = wt * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + wr * pp;
    s = off ? 0.0 : sqrt(s2);
    if (delta > 0.0 && s > delta) rho = delta / s;
#pragma unroll
    for (int j = 0; j < 9; ++j) L[j] = RE[j], L[9 + j] = J[j], L[18 + j] = RM[j];
    L[27] = tM[0], L[28] = tM[1], L[29] = tM[2];
    L[30] = rho * wt, L[31] = rho * wr;
#pragma unroll
    for (int j = 0; j < 6; ++j) L[32 + j] = r[j];
  }
  if (resid)
#pragma unroll
    for (int j = 0; j < 6; ++j) resid[e * 6 + j] = r[j];
  ecost[e] = (rho * (1.0 - 0.5 * rho)) * (s * s);
  if (rho_out) rho_out[e] = rho;
  if (s_out) s_out[e] = s;
  edge_status[e] = status;
}

// ------------------------------------------------------------------ per (edge, side) pieces
struct PgEdge {
  double RE[9], J[9], RM[9], tM[3], wt, wr, r[6];
};
__device__ static inline void pg_load(const double* __restrict__ L, PgEdge& g) {
#pragma unroll
  for (int j = 0; j < 9; ++j) g.RE[j] = L[j], g.J[j] = L[9 + j], g.RM[j] = L[18 + j];
  g.tM[0] = L[27], g.tM[1] = L[28], g.tM[2] = L[29];
  g.wt = L[30], g.wr = L[31];
#pragma unroll
  for (int j = 0; j < 6; ++j) g.r[j] = L[32 + j];
}
// u = J_a pa + J_b pb
__device__ static inline void pg_apply(const PgEdge& g, const double* pa, const double* pb, double* u) {
  double c[3], v[3], w[3];
  cross3(g.tM, pa + 3, c);
#pragma unroll
  for (int i = 0; i < 3; ++i) c[i] -= pa[i];
  m3_tvec(g.RM, c, v);
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] += pb[i];
  m3_vec(g.RE, v, u);
  m3_tvec(g.RM, pa + 3, w);
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = pb[3 + i] - w[i];
  m3_vec(g.J, w, u + 3);
}
// acc += J_side^T y
__device__ static inline void pg_transpose_add(const PgEdge& g, int side, const double* y, double* acc) {
  double q[3], h[3];
  m3_tvec(g.RE, y, q);
  m3_tvec(g.J, y + 3, h);
  if (side) {
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] += q[i], acc[3 + i] += h[i];
  } else {
    double Q[3], c[3], H[3];
    m3_vec(g.RM, q, Q);
    cross3(g.tM, Q, c);
    m3_vec(g.RM, h, H);
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] -= Q[i], acc[3 + i] -= c[i] + H[i];
  }
}

// apply (L D L^T)^-1 stored as 15 entries of L (row-wise below the diagonal) and 6 of 1/d
__device__ static inline void pg_precond(const double* __restrict__ F, const double* r, double* z) {
  double x[6];
  int e = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double y = r[i];
#pragma unroll
    for (int k = 0; k < i; ++k) y -= F[e++] * x[k];
    x[i] = y;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] *= F[15 + i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double y = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) y -= F[k * (k - 1) / 2 + i] * x[k];
    x[i] = y;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) z[i] = x[i];
}

// ------------------------------------------------------------------ gradient, diagonal blocks, PCG start: one node per lane
// SOLVE = 0: the gradient of every node (no gauge) and the cost partials (egonn_pose_graph_cost)
// SOLVE = 1: gauge applied, H_ii + lambda I factored, x = 0, r = -g, z = M^-1 r, partials of r.z and of max |g|
template <int SOLVE>
__global__ __launch_bounds__(PG_WG) void pg_setup_kernel(PgState* __restrict__ st, int32_t n, const int32_t* __restrict__ row_start,
                                                         const uint32_t* __restrict__ inc, const uint8_t* __restrict__ fixed,
                                                         const double* __restrict__ lin0, const double* __restrict__ lin1,
                                                         const double* __restrict__ ecost, double* __restrict__ grad,
                                                         double* __restrict__ fac, double* __restrict__ x, double* __restrict__ r, double* __restrict__ z, double* __restrict__ rz0p,
                                                         double* __restrict__ rzp, double* __restrict__ gmaxp,
                                                         double* __restrict__ costp, int32_t* __restrict__ graph_status) {
  if (st->done) return;
  const int64_t i = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  const double* lin = st->cur ? lin1 : lin0;
  double g[6] = {0, 0, 0, 0, 0, 0}, A[6][6], cost = 0.0;
#pragma unroll
  for (int a = 0; a < 6; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) A[a][b] = 0.0;
  const bool fx = SOLVE && i < n && fixed[i];
  if (i < n) {
    for (int32_t at = row_start[i]; at < row_start[i + 1]; ++at) {
      const uint32_t v = inc[at];
      const int64_t e = v >> 1;
      const int side = v & 1;
      PgEdge ed;
      pg_load(lin + e * PG_LIN, ed);
      double y[6];
#pragma unroll
      for (int j = 0; j < 3; ++j) y[j] = ed.wt * ed.r[j], y[3 + j] = ed.wr * ed.r[3 + j];
      pg_transpose_add(ed, side, y, g);
      if (!SOLVE && side == 0) cost += ecost[e];
      if (SOLVE) {
        double G[9];                                                   // wr Jri^T Jri, for side a turned by R_M
        m3_tmul(ed.J, ed.J, G);
        if (side == 0) {
          double T1[9], RMt[9];
          m3_mul(ed.RM, G, T1);
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) RMt[3 * a + b] = ed.RM[3 * b + a];
          m3_mul(T1, RMt, G);
          const double* t = ed.tM;
          const double tt = t[0] * t[0] + t[1] * t[1] + t[2] * t[2];
#pragma unroll
          for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) A[3 + a][3 + b] += ed.wt * ((a == b ? tt : 0.0) - t[a] * t[b]);
          // -wt [t]x in the (v, w) block, its transpose below
          A[0][4] += ed.wt * t[2], A[0][5] -= ed.wt * t[1], A[1][3] -= ed.wt * t[2];
          A[1][5] += ed.wt * t[0], A[2][3] += ed.wt * t[1], A[2][4] -= ed.wt * t[0];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          A[a][a] += ed.wt;
#pragma unroll
          for (int b = 0; b < 3; ++b) A[3 + a][3 + b] += ed.wr * G[3 * a + b];
        }
      }
    }
  }
  if (!SOLVE) {
    if (i < n)
#pragma unroll
      for (int j = 0; j < 6; ++j) grad[i * 6 + j] = g[j];
    cost = pg_wave_sum(cost);
    if (threadIdx.x == 0) costp[blockIdx.x] = cost;
    return;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) st->flag_a = 0, st->flag_b = 0;     // read by the PCG launches only
  double rr[6] = {0, 0, 0, 0, 0, 0}, zz[6] = {0, 0, 0, 0, 0, 0}, gmax = 0.0, rz = 0.0;
  if (i < n) {
    double F[21];
    bool ok = !fx;
    const double lambda = st->lambda;
    if (ok) {
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 3; b < 6; ++b) A[b][a] = A[a][b];
      double Lm[6][6], d[6];
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const double ajj = A[j][j] + lambda;
        double dj = ajj;
#pragma unroll
        for (int k = 0; k < j; ++k) dj -= (Lm[j][k] * Lm[j][k]) * d[k];
        ok = ok && dj > 0x1p-40 * ajj;                                  // the pivot rule of icp_plane_step; false for NaN
        d[j] = ok ? dj : 1.0;
#pragma unroll
        for (int a = j + 1; a < 6; ++a) {
          double l = A[a][j];
#pragma unroll
          for (int k = 0; k < j; ++k) l -= (Lm[a][k] * Lm[j][k]) * d[k];
          Lm[a][j] = l / d[j];
        }
      }
      int e = 0;
#pragma unroll
      for (int a = 1; a < 6; ++a)
#pragma unroll
        for (int b = 0; b < a; ++b) F[e++] = Lm[a][b];
#pragma unroll
      for (int j = 0; j < 6; ++j) F[15 + j] = 1.0 / d[j];
      if (!ok) atomicOr(graph_status, EGONN_PG_STATUS_PIVOT);
    }
    if (!ok) {                                                           // identity block: a fixed node or a failed pivot
#pragma unroll
      for (int j = 0; j < 15; ++j) F[j] = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) F[15 + j] = 1.0;
    }
#pragma unroll
    for (int j = 0; j < 21; ++j) fac[i * 21 + j] = F[j];
    if (!fx) {
#pragma unroll
      for (int j = 0; j < 6; ++j) rr[j] = -g[j], gmax = fmax(gmax, fabs(g[j]));
      pg_precond(F, rr, zz);
#pragma unroll
      for (int j = 0; j < 6; ++j) rz += rr[j] * zz[j];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) x[i * 6 + j] = 0.0, r[i * 6 + j] = rr[j], z[i * 6 + j] = zz[j];
  }
  rz = pg_wave_sum(rz);
  gmax = pg_wave_max(gmax);
  if (threadIdx.x == 0) rz0p[blockIdx.x] = rz, rzp[blockIdx.x] = rz, gmaxp[blockIdx.x] = gmax;
}

// ------------------------------------------------------------------ PCG iteration k, first half: p = z + beta p_old, q = (H + lambda) p
// SEAM: q = (J^T W J + lambda) p_in on the free nodes with nothing else read or written (egonn_pose_graph_hessvec)
template <int SEAM>
__global__ __launch_bounds__(PG_WG) void pg_pcg_a_kernel(PgState* __restrict__ st, int k, int32_t n, int nwg, double tol2,
                                                         double lambda_seam, const int32_t* __restrict__ row_start,
                                                         const uint32_t* __restrict__ inc, const int32_t* __restrict__ ab,
                                                         const uint8_t* __restrict__ fixed, const double* __restrict__ lin0,
                                                         const double* __restrict__ lin1, const double* __restrict__ z,
                                                         const double* __restrict__ p_old, double* __restrict__ p_new,
                                                         double* __restrict__ q, const double* __restrict__ rz0p,
                                                         const double* __restrict__ rz_new_p, const double* __restrict__ rz_old_p,
                                                         double* __restrict__ pqp) {
  double beta = 0.0, lambda = lambda_seam;
  if (!SEAM) {
    if (st->done || st->flag_b) {
      if (blockIdx.x == 0 && threadIdx.x == 0) st->flag_a = 1;
      return;
    }
    const double rz0 = pg_sum(rz0p, nwg), rz_new = pg_sum(rz_new_p, nwg);
    if (!(rz_new > tol2 * rz0)) {                                       // converged (or NaN): every workgroup sees the same sums
      if (blockIdx.x == 0 && threadIdx.x == 0) st->flag_a = 1;
      return;
    }
    if (k > 0) beta = rz_new / pg_sum(rz_old_p, nwg);
    lambda = st->lambda;
  }
  const double* lin = st->cur ? lin1 : lin0;
  const int64_t i = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  auto direction = [&](int64_t j, double* p) {                          // p_new of node j, whoever owns it
    const bool f = fixed[j];
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      const double zj = z[j * 6 + c];
      p[c] = f ? 0.0 : (SEAM || k == 0 ? zj : zj + beta * p_old[j * 6 + c]);
    }
  };
  double pq = 0.0;
  if (i < n) {
    double pi[6], acc[6] = {0, 0, 0, 0, 0, 0};
    direction(i, pi);
    if (!fixed[i]) {
      for (int32_t at = row_start[i]; at < row_start[i + 1]; ++at) {
        const uint32_t v = inc[at];
        const int64_t e = v >> 1;
        const int side = v & 1;
        PgEdge ed;
        pg_load(lin + e * PG_LIN, ed);
        double po[6], u[6];
        direction(ab[2 * e + (side ^ 1)], po);
        pg_apply(ed, side ? po : pi, side ? pi : po, u);
#pragma unroll
        for (int j = 0; j < 3; ++j) u[j] *= ed.wt, u[3 + j] *= ed.wr;
        pg_transpose_add(ed, side, u, acc);
      }
#pragma unroll
      for (int j = 0; j < 6; ++j) acc[j] += lambda * pi[j], pq += pi[j] * acc[j];
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      q[i * 6 + j] = acc[j];
      if (!SEAM) p_new[i * 6 + j] = pi[j];
    }
  }
  if (!SEAM) {
    pq = pg_wave_sum(pq);
    if (threadIdx.x == 0) pqp[blockIdx.x] = pq;
  }
}

// second half: alpha = r.z / p.q, x += alpha p, r -= alpha q, z = M^-1 r, partials of the new r.z
__global__ __launch_bounds__(PG_WG) void pg_pcg_b_kernel(PgState* __restrict__ st, int32_t n, int nwg, const double* __restrict__ fac,
                                                         const double* __restrict__ p, const double* __restrict__ q,
                                                         double* __restrict__ x, double* __restrict__ r, double* __restrict__ z,
                                                         const double* __restrict__ pqp, const double* __restrict__ rz_cur_p,
                                                         double* __restrict__ rz_next_p) {
  if (st->done || st->flag_a) {
    if (blockIdx.x == 0 && threadIdx.x == 0) st->flag_b = 1;
    return;
  }
  const double pq = pg_sum(pqp, nwg), rz = pg_sum(rz_cur_p, nwg);
  if (!(pq > 0.0)) {                                                    // breakdown: x stays what it is
    if (blockIdx.x == 0 && threadIdx.x == 0) st->flag_b = 1;
    return;
  }
  const double alpha = rz / pq;
  const int64_t i = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  double part = 0.0;
  if (i < n) {
    double rr[6], zz[6], F[21];
#pragma unroll
    for (int j = 0; j < 21; ++j) F[j] = fac[i * 21 + j];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      x[i * 6 + j] += alpha * p[i * 6 + j];
      rr[j] = r[i * 6 + j] - alpha * q[i * 6 + j];
    }
    pg_precond(F, rr, zz);
#pragma unroll
    for (int j = 0; j < 6; ++j) r[i * 6 + j] = rr[j], z[i * 6 + j] = zz[j], part += rr[j] * zz[j];
  }
  part = pg_wave_sum(part);
  if (threadIdx.x == 0) rz_next_p[blockIdx.x] = part;
}

// ------------------------------------------------------------------ candidate poses
__global__ __launch_bounds__(PG_WG) void pg_retract_kernel(const PgState* __restrict__ st, int32_t n, double* __restrict__ X0,
                                                           double* __restrict__ X1, const double* __restrict__ x) {
  if (st->done) return;
  const int64_t i = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  if (i >= n) return;
  const double* src = (st->cur ? X1 : X0) + i * 16;
  double* dst = (st->cur ? X0 : X1) + i * 16;
  double d[6];
  bool any = false;
#pragma unroll
  for (int j = 0; j < 6; ++j) d[j] = x[i * 6 + j], any = any || d[j] != 0.0;
  if (!any) {                                                           // bit-unchanged
#pragma unroll
    for (int j = 0; j < 16; ++j) dst[j] = src[j];
    return;
  }
  double R[9], t[3], Ex[9], Rn[9], G[9], Ro[9], Rv[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) R[3 * a + b] = src[4 * a + b];
    t[a] = src[4 * a + 3];
  }
  const double w0 = d[3], w1 = d[4], w2 = d[5], th2 = w0 * w0 + w1 * w1 + w2 * w2, th = sqrt(th2);
  double sa, sb;                                                        // sin(th) / th and (1 - cos th) / th^2 = 2 sin^2(th / 2) / th^2
  if (th < 1e-8) {
    sa = 1.0 - th2 / 6.0, sb = 0.5;
  } else {
    const double h = sin(0.5 * th);
    sa = sin(th) / th, sb = 2.0 * (h * h) / th2;
  }
  Ex[0] = 1.0 - sb * (w1 * w1 + w2 * w2), Ex[1] = -sa * w2 + sb * w0 * w1, Ex[2] = sa * w1 + sb * w0 * w2;
  Ex[3] = sa * w2 + sb * w0 * w1, Ex[4] = 1.0 - sb * (w0 * w0 + w2 * w2), Ex[5] = -sa * w0 + sb * w1 * w2;
  Ex[6] = -sa * w1 + sb * w0 * w2, Ex[7] = sa * w0 + sb * w1 * w2, Ex[8] = 1.0 - sb * (w0 * w0 + w1 * w1);
  m3_mul(R, Ex, Rn);
  m3_tmul(Rn, Rn, G);                                                   // one Newton-Schulz step: Rn (3 I - Rn^T Rn) / 2
#pragma unroll
  for (int j = 0; j < 9; ++j) G[j] = 0.5 * ((j % 4 == 0 ? 3.0 : 0.0) - G[j]);
  m3_mul(Rn, G, Ro);
  m3_vec(R, d, Rv);
#pragma unroll
  for (int a = 0; a < 3; ++a) {
#pragma unroll
    for (int b = 0; b < 3; ++b) dst[4 * a + b] = Ro[3 * a + b];
    dst[4 * a + 3] = t[a] + Rv[a];
  }
#pragma unroll
  for (int j = 12; j < 16; ++j) dst[j] = src[j];
}

// the cost of a linearisation, grouped by node (the terms of the edges a node is side a of), so that an edge that is switched
// off does not move any other term into another partial
__global__ __launch_bounds__(PG_WG) void pg_node_cost_kernel(const PgState* __restrict__ st, int32_t n, const int32_t* __restrict__ row_start,
                                                             const uint32_t* __restrict__ inc, const double* __restrict__ ecost,
                                                             double* __restrict__ costp) {
  if (st->done) return;
  const int64_t i = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  double c = 0.0;
  if (i < n)
    for (int32_t at = row_start[i]; at < row_start[i + 1]; ++at) {
      const uint32_t v = inc[at];
      if (!(v & 1)) c += ecost[v >> 1];
    }
  c = pg_wave_sum(c);
  if (threadIdx.x == 0) costp[blockIdx.x] = c;
}

// one workgroup.  first: the cost of the start.  Otherwise outer step st->iter: accept when the cost decreases
__global__ __launch_bounds__(PG_WG) void pg_decide_kernel(PgState* __restrict__ st, int first, int nwg, const double* __restrict__ costp,
                                                          const double* __restrict__ gmaxp, double lambda_min, double lambda_max,
                                                          double rel_tol, double grad_tol, double* __restrict__ cost_trace,
                                                          int32_t* __restrict__ accept_trace) {
  if (st->done) return;
  const double cc = pg_sum(costp, nwg);
  double gmax = 0.0;
  if (!first) {
    for (int j = threadIdx.x; j < nwg; j += PG_WG) gmax = fmax(gmax, gmaxp[j]);
    gmax = pg_wave_max(gmax);
  }
  if (threadIdx.x != 0) return;
  if (first) {
    st->cost = cc;
    cost_trace[0] = cc;
    return;
  }
  const int k = st->iter;
  const double c = st->cost;
  int done = 0;
  if (cc < c) {                                                         // false for NaN
    done = (c - cc) < rel_tol * c;
    st->cost = cc;
    st->cur ^= 1;
    st->lambda = fmax(st->lambda / 10.0, lambda_min);
    st->accepted += 1;
    if (accept_trace) accept_trace[k] = 1;
  } else {
    st->lambda *= 10.0;
    if (accept_trace) accept_trace[k] = 0;
  }
  st->iter = k + 1;
  cost_trace[k + 1] = st->cost;
  if (done || st->lambda > lambda_max || gmax <= grad_tol) st->done = 1;
}

__global__ __launch_bounds__(PG_WG) void pg_finish_kernel(const PgState* __restrict__ st, int32_t n, const double* __restrict__ X0,
                                                          const double* __restrict__ X1, double* __restrict__ poses_out,
                                                          int32_t* __restrict__ counters, double* __restrict__ lambda_out) {
  const int64_t j = (int64_t)blockIdx.x * PG_WG + threadIdx.x;
  if (j < (int64_t)n * 16) poses_out[j] = (st->cur ? X1 : X0)[j];
  if (j == 0) {
    counters[0] = st->iter, counters[1] = st->accepted;
    *lambda_out = st->lambda;
  }
}

// ------------------------------------------------------------------ the scratch span
// Every array of the plan and of the optimiser's state, carved in this order.  With scratch = nullptr only `total` means anything
struct PgSpan {
  int32_t *ab, *pstat, *row_start;                            // the plan
  double* weff;
  uint8_t* fixed;
  uint32_t* inc;
  uint64_t* keys[2];                                          // ping-pong buffers of the plan's sort
  uint32_t* vals[2];
  Arena sort_ws;
  PgState* state;                                             // the optimiser
  double *X0, *X1, *lin0, *lin1, *ecost, *fac, *x, *r, *z, *q, *p[2], *pqp, *rz0p, *rzp[2], *gmaxp, *costp;
  size_t total;
};
static bool pg_sizes_ok(int64_t n, int64_t E) { return pose_sizes_ok(n, E); }
static PgSpan pg_span(void* scratch, int64_t n, int64_t E) {
  PgSpan P;
  Carve c(scratch);
  const size_t nn = (size_t)n, ee = (size_t)(E > 0 ? E : 1), nwg = (size_t)cdiv(n, PG_WG);
  P.ab = c.take<int32_t>(ee * 2), P.weff = c.take<double>(ee * 2), P.pstat = c.take<int32_t>(ee), P.fixed = c.take<uint8_t>(nn);
  P.row_start = c.take<int32_t>(nn + 1), P.inc = c.take<uint32_t>(ee * 2);
  for (int k = 0; k < 2; ++k) P.keys[k] = c.take<uint64_t>(ee * 2);
  for (int k = 0; k < 2; ++k) P.vals[k] = c.take<uint32_t>(ee * 2);
  P.sort_ws = c.sort_arena(radix_sort_scratch_bytes(2 * (int64_t)ee));
  P.state = c.take<PgState>(1);
  P.X0 = c.take<double>(nn * 16), P.X1 = c.take<double>(nn * 16), P.lin0 = c.take<double>(ee * PG_LIN), P.lin1 = c.take<double>(ee * PG_LIN);
  P.ecost = c.take<double>(ee), P.fac = c.take<double>(nn * 21);
  for (double** v : {&P.x, &P.r, &P.z, &P.q, &P.p[0], &P.p[1]}) *v = c.take<double>(nn * 6);
  for (double** v : {&P.pqp, &P.rz0p, &P.rzp[0], &P.rzp[1], &P.gmaxp, &P.costp}) *v = c.take<double>(nwg);
  P.total = c.total();
  return P;
}

static int pg_check_span(const char* who, int64_t n, int64_t E, void* scratch, int64_t scratch_bytes, PgSpan* P) {
  EGONN_REQUIRE(pg_sizes_ok(n, E), EGONN_ERR_INVALID, "%s: n=%lld E=%lld outside 1 <= n < 2^31 - 1, 0 <= E < 2^30", who, (long long)n,
                (long long)E);
  *P = pg_span(scratch, n, E);
  return span_check(who, scratch, scratch_bytes, P->total);
}
static inline bool pg_tol_ok(double v) { return v >= 0.0 && v < INFINITY; }

static inline unsigned pg_grid(int64_t items) { return (unsigned)cdiv(items > 0 ? items : 1, PG_WG); }

API int64_t egonn_pose_graph_scratch_bytes(int64_t n, int64_t E, int pcg_iterations) {
  if (!pg_sizes_ok(n, E) || pcg_iterations < 1) return -1;
  return (int64_t)pg_span(nullptr, n, E).total;                   // the PCG keeps no per-iteration record: the budget adds nothing
}

API int egonn_pose_graph_odometry(const double* poses, int64_t n, double* Z, int32_t* edge_index, void* stream) {
  EGONN_REQUIRE(n >= 1 && n < (1ll << 31) - 1, EGONN_ERR_INVALID, "pose_graph_odometry: n=%lld outside 1 <= n < 2^31 - 1", (long long)n);
  EGONN_REQUIRE(poses && (n == 1 || (Z && edge_index)), EGONN_ERR_INVALID, "pose_graph_odometry: null pointer");
  if (n == 1) return EGONN_OK;
  hipLaunchKernelGGL(pg_odometry_kernel, dim3(pg_grid(n - 1)), dim3(PG_WG), 0, (hipStream_t)stream, poses, (int32_t)(n - 1), Z,
                     edge_index);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_pose_graph_plan(const int32_t* edge_index, const double* Z, const double* weights, const uint8_t* fixed, int64_t n,
                              int64_t E, int32_t* edge_status, int32_t* graph_status, void* scratch, int64_t scratch_bytes,
                              void* stream) {
  PgSpan P;
  EGONN_TRY(pg_check_span("pose_graph_plan", n, E, scratch, scratch_bytes, &P));
  EGONN_REQUIRE(graph_status && (E == 0 || (edge_index && Z && edge_status)), EGONN_ERR_INVALID, "pose_graph_plan: null pointer");
  hipStream_t st = (hipStream_t)stream;
  uint64_t *keys0 = P.keys[0], *keys1 = P.keys[1], *kres = nullptr;
  uint32_t *vals0 = P.vals[0], *vals1 = P.vals[1], *vres = nullptr;
  HIP_CHECK(hipMemsetAsync(graph_status, 0, sizeof(int32_t), st));
  if (E > 0) {
    hipLaunchKernelGGL(pg_validate_kernel, dim3(pg_grid(E)), dim3(PG_WG), 0, st, edge_index, Z, weights, (int32_t)n, (int32_t)E, P.ab,
                       P.weff, P.pstat, edge_status, keys0, vals0);
    int nbits = 1;
    while ((n >> nbits) != 0) ++nbits;                       // keys are 0 .. n
    kres = keys1, vres = vals1;
    EGONN_TRY(radix_sort_pairs(P.sort_ws, keys0, vals0, keys1, vals1, 2 * E, nbits, st, nullptr, &kres, &vres));
  }
  const int64_t threads = 2 * E > n + 1 ? 2 * E : n + 1;
  hipLaunchKernelGGL(pg_csr_kernel, dim3(pg_grid(threads)), dim3(PG_WG), 0, st, kres, vres, (int32_t)(2 * E), (int32_t)n, fixed,
                     P.row_start, P.inc, P.fixed, graph_status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_pose_graph_cost(const double* poses, int64_t n, int64_t E, const double* Z, double robust_delta, double* cost,
                              double* residuals, double* rho, double* s, double* gradient, int32_t* edge_status, void* scratch,
                              int64_t scratch_bytes, void* stream) {
  PgSpan P;
  EGONN_TRY(pg_check_span("pose_graph_cost", n, E, scratch, scratch_bytes, &P));
  EGONN_REQUIRE(poses && cost && gradient && (E == 0 || (Z && residuals && rho && s && edge_status)), EGONN_ERR_INVALID,
                "pose_graph_cost: null pointer");
  EGONN_REQUIRE(pg_tol_ok(robust_delta), EGONN_ERR_INVALID, "pose_graph_cost: robust_delta=%g is negative or not finite", robust_delta);
  hipStream_t st = (hipStream_t)stream;
  const int nwg = (int)cdiv(n, PG_WG);
  hipLaunchKernelGGL(pg_init_kernel, dim3(1), dim3(PG_WG), 0, st, P.state, 0.0, (double*)nullptr, (int32_t*)nullptr, 0);
  if (E > 0)
    hipLaunchKernelGGL(pg_linearize_kernel, dim3(pg_grid(E)), dim3(PG_WG), 0, st, P.state, poses, poses, 0, 1, (int32_t)E, P.ab, P.weff,
                       P.pstat, Z, robust_delta, P.lin0, P.lin1, residuals, P.ecost, rho, s, edge_status);
  hipLaunchKernelGGL(pg_setup_kernel<0>, dim3(nwg), dim3(PG_WG), 0, st, P.state, (int32_t)n, P.row_start, P.inc, P.fixed, P.lin0, P.lin1,
                     P.ecost, gradient, P.fac, P.x, P.r, P.z, P.rz0p, P.rzp[0], P.gmaxp, P.costp, (int32_t*)nullptr);
  hipLaunchKernelGGL(pg_decide_kernel, dim3(1), dim3(PG_WG), 0, st, P.state, 1, nwg, P.costp, P.gmaxp, 0.0, 0.0, 0.0, 0.0, cost,
                     (int32_t*)nullptr);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_pose_graph_hessvec(const double* poses, int64_t n, int64_t E, const double* Z, double robust_delta, double lambda,
                                 const double* p, double* out, int32_t* edge_status, void* scratch, int64_t scratch_bytes,
                                 void* stream) {
  PgSpan P;
  EGONN_TRY(pg_check_span("pose_graph_hessvec", n, E, scratch, scratch_bytes, &P));
  EGONN_REQUIRE(poses && p && out && (E == 0 || (Z && edge_status)), EGONN_ERR_INVALID, "pose_graph_hessvec: null pointer");
  EGONN_REQUIRE(pg_tol_ok(robust_delta) && pg_tol_ok(lambda), EGONN_ERR_INVALID,
                "pose_graph_hessvec: robust_delta=%g or lambda=%g is negative or not finite", robust_delta, lambda);
  hipStream_t st = (hipStream_t)stream;
  const int nwg = (int)cdiv(n, PG_WG);
  hipLaunchKernelGGL(pg_init_kernel, dim3(1), dim3(PG_WG), 0, st, P.state, lambda, (double*)nullptr, (int32_t*)nullptr, 0);
  if (E > 0)
    hipLaunchKernelGGL(pg_linearize_kernel, dim3(pg_grid(E)), dim3(PG_WG), 0, st, P.state, poses, poses, 0, 1, (int32_t)E, P.ab, P.weff,
                       P.pstat, Z, robust_delta, P.lin0, P.lin1, (double*)nullptr, P.ecost, (double*)nullptr, (double*)nullptr, edge_status);
  hipLaunchKernelGGL(pg_pcg_a_kernel<1>, dim3(nwg), dim3(PG_WG), 0, st, P.state, 0, (int32_t)n, nwg, 0.0, lambda, P.row_start, P.inc, P.ab,
                     P.fixed, P.lin0, P.lin1, p, p, (double*)nullptr, out, P.rz0p, P.rzp[0], P.rzp[1], P.pqp);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_pose_graph_optimize(const double* poses, int64_t n, int64_t E, const double* Z, double robust_delta, int max_iterations,
                                  int pcg_iterations, double pcg_tol, double lambda_init, double lambda_min, double lambda_max,
                                  double rel_tol, double grad_tol, double* poses_out, double* cost_trace, int32_t* accept_trace,
                                  int32_t* counters, double* lambda_out, int32_t* edge_status, int32_t* graph_status, void* scratch,
                                  int64_t scratch_bytes, void* stream) {
  PgSpan P;
  EGONN_TRY(pg_check_span("pose_graph_optimize", n, E, scratch, scratch_bytes, &P));
  EGONN_REQUIRE(poses && poses_out && cost_trace && accept_trace && counters && lambda_out && graph_status &&
                    (E == 0 || (Z && edge_status)),
                EGONN_ERR_INVALID, "pose_graph_optimize: null pointer");
  EGONN_REQUIRE(max_iterations >= 1 && pcg_iterations >= 1, EGONN_ERR_INVALID,
                "pose_graph_optimize: max_iterations=%d pcg_iterations=%d must be positive", max_iterations, pcg_iterations);
  EGONN_REQUIRE(pg_tol_ok(robust_delta) && pg_tol_ok(pcg_tol) && pg_tol_ok(rel_tol) && pg_tol_ok(grad_tol), EGONN_ERR_INVALID,
                "pose_graph_optimize: a tolerance is negative or not finite (robust_delta=%g pcg_tol=%g rel_tol=%g grad_tol=%g)",
                robust_delta, pcg_tol, rel_tol, grad_tol);
  EGONN_REQUIRE(lambda_min > 0.0 && lambda_init >= lambda_min && lambda_max >= lambda_init && lambda_max < INFINITY, EGONN_ERR_INVALID,
                "pose_graph_optimize: 0 < lambda_min <= lambda_init <= lambda_max < inf expected, got %g, %g, %g", lambda_min,
                lambda_init, lambda_max);
  hipStream_t st = (hipStream_t)stream;
  const int nwg = (int)cdiv(n, PG_WG);
  const int32_t nn = (int32_t)n, ee = (int32_t)E;
  const dim3 gn(nwg), ge(pg_grid(E)), blk(PG_WG);
  auto linearize = [&](int which, int first) {
    if (E > 0)
      hipLaunchKernelGGL(pg_linearize_kernel, ge, blk, 0, st, P.state, P.X0, P.X1, which, first, ee, P.ab, P.weff, P.pstat, Z,
                         robust_delta, P.lin0, P.lin1, (double*)nullptr, P.ecost, (double*)nullptr, (double*)nullptr, edge_status);
    hipLaunchKernelGGL(pg_node_cost_kernel, gn, blk, 0, st, P.state, nn, P.row_start, P.inc, P.ecost, P.costp);
  };
  HIP_CHECK(hipMemcpyAsync(P.X0, poses, (size_t)n * 128, hipMemcpyDeviceToDevice, st));
  hipLaunchKernelGGL(pg_init_kernel, dim3(1), blk, 0, st, P.state, lambda_init, cost_trace, accept_trace, max_iterations);
  linearize(0, 1);
  hipLaunchKernelGGL(pg_decide_kernel, dim3(1), blk, 0, st, P.state, 1, nwg, P.costp, P.gmaxp, lambda_min, lambda_max, rel_tol, grad_tol,
                     cost_trace, accept_trace);
  const double tol2 = pcg_tol * pcg_tol;
  for (int it = 0; it < max_iterations; ++it) {
    hipLaunchKernelGGL(pg_setup_kernel<1>, gn, blk, 0, st, P.state, nn, P.row_start, P.inc, P.fixed, P.lin0, P.lin1, P.ecost,
                       (double*)nullptr, P.fac, P.x, P.r, P.z, P.rz0p, P.rzp[0], P.gmaxp, P.costp, graph_status);
    for (int k = 0; k < pcg_iterations; ++k) {
      hipLaunchKernelGGL(pg_pcg_a_kernel<0>, gn, blk, 0, st, P.state, k, nn, nwg, tol2, 0.0, P.row_start, P.inc, P.ab, P.fixed, P.lin0,
                         P.lin1, P.z, P.p[k & 1], P.p[(k + 1) & 1], P.q, P.rz0p, P.rzp[k & 1], P.rzp[(k + 1) & 1], P.pqp);
      hipLaunchKernelGGL(pg_pcg_b_kernel, gn, blk, 0, st, P.state, nn, nwg, P.fac, P.p[(k + 1) & 1], P.q, P.x, P.r, P.z, P.pqp,
                         P.rzp[k & 1], P.rzp[(k + 1) & 1]);
    }
    hipLaunchKernelGGL(pg_retract_kernel, gn, blk, 0, st, P.state, nn, P.X0, P.X1, P.x);
    linearize(1, 0);
    hipLaunchKernelGGL(pg_decide_kernel, dim3(1), blk, 0, st, P.state, 0, nwg, P.costp, P.gmaxp, lambda_min, lambda_max, rel_tol,
                       grad_tol, cost_trace, accept_trace);
  }
  hipLaunchKernelGGL(pg_finish_kernel, dim3(pg_grid(n * 16)), blk, 0, st, P.state, nn, P.X0, P.X1, poses_out, counters, lambda_out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn
