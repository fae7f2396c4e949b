// The 6-DoF Gauss-Newton step shared by the point-to-plane ICP (icp.hip) and the NDT registration (ndt.hip): a 6 x 6 normal
// system from its packed sums, solved by LDL^T without pivoting, and the small-angle update it stands for.  Every operation is
// the IEEE operation that is written (contraction off), so both callers get the same bits from the same sums.
#pragma once

#pragma clang fp contract(off)

namespace egonn {

// Solves A x = -b (A from its 21 upper entries row by row at s[2..22], b at s[23..28]) by LDL^T without pivoting.  False, with
// nothing to rely on in x, when a pivot d_i is not > 2^-40 A_ii (A's own diagonal: fp64 leaves ~2^-52 relative rounding in a
// pivot, twelve bits above that separate a rank-deficient scene from rounding noise) or x is not finite.
__device__ static bool icp_plane_solve(const double* __restrict__ s, double* x) {
  double A[6][6], L[6][6], d[6];
  {
    int e = 2;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = s[e++];
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double dj = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) dj -= (L[j][k] * L[j][k]) * d[k];
    ok = ok && dj > 0x1p-40 * A[j][j];                  // false for NaN as well
    d[j] = ok ? dj : 1.0;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double l = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) l -= (L[i][k] * L[j][k]) * d[k];
      L[i][j] = l / d[j];
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {                          // L y = -b
    double y = -s[23 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) y -= L[i][k] * x[k];
    x[i] = y;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = x[i] / d[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {                         // L^T x = z
    double y = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) y -= L[k][i] * x[k];
    x[i] = y;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) ok = ok && fabs(x[i]) < INFINITY;
  return ok;
}

// U = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)] as (U[9], ut[3])
__device__ static inline void icp_plane_update(const double* x, double* U, double* ut) {
  const double sa = sin(x[0]), ca = cos(x[0]), sb = sin(x[1]), cb = cos(x[1]), sc = sin(x[2]), cc = cos(x[2]);
  U[0] = cb * cc, U[1] = (sa * sb) * cc - ca * sc, U[2] = (ca * sb) * cc + sa * sc;
  U[3] = cb * sc, U[4] = (sa * sb) * sc + ca * cc, U[5] = (ca * sb) * sc - sa * cc;
  U[6] = -sb, U[7] = sa * cb, U[8] = ca * cb;
  ut[0] = x[3], ut[1] = x[4], ut[2] = x[5];
}

// Point-to-plane step: icp_plane_solve, then icp_plane_update.  False, with nothing to rely on in U, when the solve is.
__device__ static bool icp_plane_step(const double* __restrict__ s, double* U, double* ut) {
  double x[6];
  const bool ok = icp_plane_solve(s, x);
  icp_plane_update(x, U, ut);
  return ok;
}

}  // namespace egonn
