// Eigen-decomposition of a symmetric 3 x 3 matrix by cyclic Jacobi on a fixed schedule, shared by the surface normals (icp.hip)
// and the per-voxel Gaussians of the NDT layer (ndt.hip).  Every operation is the IEEE operation that is written (contraction
// off), so both callers get the same bits from the same matrix.
#pragma once

#pragma clang fp contract(off)

namespace egonn {

// eigen-decomposition of the symmetric 3 x 3 matrix A by cyclic Jacobi, the schedule of horn_top_eigenvector (horn.h): A's diagonal
// becomes the eigenvalues, the columns of V the eigenvectors
__device__ static inline void nrm_jacobi3(double A[3][3], double V[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; ++sweep) {
    if (fabs(A[0][1]) + fabs(A[0][2]) + fabs(A[1][2]) == 0.0) break;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = i + 1; j < 3; ++j) {
        const double apq = A[i][j];
        if (apq != 0.0) {
          const double theta = (A[j][j] - A[i][i]) / (2.0 * apq);
          const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
#pragma unroll
          for (int k = 0; k < 3; ++k) {              // A <- A J
            const double aki = A[k][i], akj = A[k][j];
            A[k][i] = c * aki - s * akj;
            A[k][j] = s * aki + c * akj;
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) {              // A <- J^T A
            const double aik = A[i][k], ajk = A[j][k];
            A[i][k] = c * aik - s * ajk;
            A[j][k] = s * aik + c * ajk;
          }
          A[i][j] = A[j][i] = 0.0;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const double vki = V[k][i], vkj = V[k][j];
            V[k][i] = c * vki - s * vkj;
            V[k][j] = s * vki + c * vkj;
          }
        }
      }
  }
}

}  // namespace egonn
