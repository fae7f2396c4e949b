// Relocalisation of query scans against a resident keypoint map: the top-k candidates of the global retrieval are verified
// by keypoint registration and the one with the most inliers gives the 6-DoF pose (P_query = P_map[best] @ T, with T the
// transform of registration.hip that maps query keypoints into the candidate's frame; misc/poses.py: T_gt = inv(P_map) @ P_query).
//
//   1. egonn_match_candidates  (match.hip) mutual nearest-neighbour matching of pair p = q * k + c = (query q, map entry
//                              nn_index[q][c]), the candidate read by index from the bank: nothing is gathered.
//   2. egonn_gather_candidates the small operands of egonn_ransac_pairs / egonn_registration_finish (keypoints, counts) and
//                              the pair id of the draws, a function of (query id, map entry) and not of rank or batch.
//   3. egonn_pick_candidates   per query the total order (most inliers, lowest inlier rmse, lowest rank; invalid candidates
//                              last), the winner's pose in the map frame and the safe pick for the ICP gather.
//
// No kernel reads by an unchecked index: a candidate index outside [0, n_bank) yields an empty pair and a status bit.
#include "../../include/egonn_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int REL_WG = 256;       // lanes of the gather kernel
static constexpr int REL_PICK_WG = 64;

__global__ __launch_bounds__(REL_WG) void reloc_gather_kernel(const float* __restrict__ q_kp, const int32_t* __restrict__ q_n,
                                                              const float* __restrict__ bank_kp,
                                                              const int32_t* __restrict__ bank_n,
                                                              const int32_t* __restrict__ nn_index,
                                                              const int32_t* __restrict__ query_id, int M, int k, int n_max,
                                                              float* __restrict__ kp1, float* __restrict__ kp2,
                                                              int32_t* __restrict__ n1, int32_t* __restrict__ n2,
                                                              int32_t* __restrict__ pair_id) {
  const int p = blockIdx.x, t = threadIdx.x, q = p / k, idx = nn_index[p];
  const bool valid = idx >= 0 && idx < M;
  const float* a = q_kp + (size_t)q * n_max * 3;
  const float* b = valid ? bank_kp + (size_t)idx * n_max * 3 : nullptr;
  float* o1 = kp1 + (size_t)p * n_max * 3;
  float* o2 = kp2 + (size_t)p * n_max * 3;
  for (int e = t; e < n_max * 3; e += REL_WG) {
    o1[e] = a[e];
    o2[e] = valid ? b[e] : 0.0f;
  }
  if (t == 0) {
    n1[p] = q_n[q];
    n2[p] = valid ? bank_n[idx] : 0;
    const int64_t qid = query_id ? (int64_t)query_id[q] : (int64_t)q;
    pair_id[p] = (int32_t)((qid * 1000003ll + (int64_t)idx) & 0x3fffffffll);   // mod 2^30 (two's complement: non-negative)
  }
}

struct RelKey {
  bool valid;
  int inl;
  double rmse;
};

// a before b in the order of the rerank: a total order (the rank decides last)
__device__ static inline bool rel_before(const RelKey& a, int ra, const RelKey& b, int rb) {
  if (a.valid != b.valid) return a.valid;
  if (!a.valid) return ra < rb;
  if (a.inl != b.inl) return a.inl > b.inl;
  if (a.rmse != b.rmse) return a.rmse < b.rmse;
  return ra < rb;
}

__global__ __launch_bounds__(REL_PICK_WG) void reloc_pick_kernel(
    const int32_t* __restrict__ nn_index, int M, int k, const double* __restrict__ map_pose, const double* __restrict__ T,
    const int32_t* __restrict__ inliers, const double* __restrict__ rmse, const int32_t* __restrict__ reg_status,
    const double* __restrict__ rte, const double* __restrict__ rre, const int32_t* __restrict__ success, int min_inliers,
    int32_t* __restrict__ best_rank, int32_t* __restrict__ best_index, int32_t* __restrict__ reranked, double* __restrict__ T_rel,
    double* __restrict__ pose, int32_t* __restrict__ safe_pick, int32_t* __restrict__ best_inliers, int32_t* __restrict__ status,
    double* __restrict__ best_rte, double* __restrict__ best_rre, int32_t* __restrict__ best_success) {
  const int q = blockIdx.x, t = threadIdx.x;
  const size_t base = (size_t)q * k;
  int bits = 0, first = -1;
  for (int c = t; c < k; c += REL_PICK_WG) {
    const int idx = nn_index[base + c];
    RelKey a;
    a.valid = idx >= 0 && idx < M;
    a.inl = inliers[base + c];
    a.rmse = rmse[base + c];
    if (!a.valid) bits |= idx == -1 ? EGONN_RELOC_NO_CANDIDATE : (EGONN_RELOC_NO_CANDIDATE | EGONN_RELOC_BAD_INDEX);
    int pos = 0;
    for (int o = 0; o < k; ++o) {
      if (o == c) continue;
      const int io = nn_index[base + o];
      RelKey b;
      b.valid = io >= 0 && io < M;
      b.inl = inliers[base + o];
      b.rmse = rmse[base + o];
      pos += rel_before(b, o, a, c) ? 1 : 0;
    }
    reranked[base + pos] = a.valid ? idx : -1;
    if (pos == 0) first = c;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bits |= __shfl_xor(bits, o, 64);
  if (first < 0) return;   // exactly one lane holds the head of the order
  const int idx = nn_index[base + first];
  const bool ok = idx >= 0 && idx < M && !(reg_status[base + first] & EGONN_REG_STATUS_NO_MODEL) &&
                  inliers[base + first] >= min_inliers;
  double R[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1}, Pq[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  if (ok) {
    const double* A = map_pose + (size_t)idx * 16;
    const double* B = T + (base + first) * 16;
#pragma unroll
    for (int e = 0; e < 16; ++e) R[e] = B[e];
    // affine product: rows 0..2 of A times B with B's last row taken as 0 0 0 1; three terms summed left to right
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) Pq[r * 4 + c] = A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c] + A[r * 4 + 2] * B[8 + c];
      Pq[r * 4 + 3] = A[r * 4] * B[3] + A[r * 4 + 1] * B[7] + A[r * 4 + 2] * B[11] + A[r * 4 + 3];
    }
  }
  for (int e = 0; e < 16; ++e) {
    T_rel[(size_t)q * 16 + e] = R[e];
    pose[(size_t)q * 16 + e] = Pq[e];
  }
  const int head = nn_index[base];
  best_rank[q] = ok ? first : -1;
  best_index[q] = ok ? idx : -1;
  safe_pick[q] = ok ? idx : clipi(head, M - 1);
  best_inliers[q] = ok ? inliers[base + first] : 0;
  status[q] = bits | (ok ? 0 : EGONN_RELOC_UNVERIFIED);
  if (best_rte) best_rte[q] = ok && rte ? rte[base + first] : -1.0;
  if (best_rre) best_rre[q] = ok && rre ? rre[base + first] : -1.0;
  if (best_success) best_success[q] = ok && success ? success[base + first] : 0;
}

int rel_check_shape(const char* who, int Q, int k, int M, int n_max) {
  EGONN_REQUIRE(Q >= 0 && k >= 1 && k <= REL_MAX_K && (int64_t)Q * k <= KP_MAX_PAIRS, EGONN_ERR_INVALID,
                "%s: bad shape (n_queries=%d, k=%d; 1 <= k <= %d, n_queries * k <= 2^20)", who, Q, k, REL_MAX_K);
  EGONN_REQUIRE(M >= 1, EGONN_ERR_INVALID, "%s: the map needs at least one entry (n_bank=%d)", who, M);
  EGONN_REQUIRE(n_max >= 1 && n_max <= KP_MAX_N, EGONN_ERR_INVALID, "%s: bad shape (n_max=%d; 1 <= n_max <= %d)", who, n_max,
                KP_MAX_N);
  return EGONN_OK;
}

}  // namespace egonn

using namespace egonn;

API int egonn_gather_candidates(const float* q_kp, const int32_t* q_n, const float* bank_kp, const int32_t* bank_n,
                                const int32_t* nn_index, const int32_t* query_id, int n_queries, int k, int n_bank, int n_max,
                                float* kp1, float* kp2, int32_t* n1, int32_t* n2, int32_t* pair_id, void* stream) {
  EGONN_TRY(rel_check_shape("gather_candidates", n_queries, k, n_bank, n_max));
  EGONN_REQUIRE(q_kp && q_n && bank_kp && bank_n && nn_index && kp1 && kp2 && n1 && n2 && pair_id, EGONN_ERR_INVALID,
                "gather_candidates: null pointer");
  if (n_queries == 0) return EGONN_OK;
  hipLaunchKernelGGL(reloc_gather_kernel, dim3((unsigned)(n_queries * k)), dim3(REL_WG), 0, (hipStream_t)stream, q_kp, q_n, bank_kp,
                     bank_n, nn_index, query_id, n_bank, k, n_max, kp1, kp2, n1, n2, pair_id);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

API int egonn_pick_candidates(const int32_t* nn_index, int n_queries, int k, int n_bank, const double* map_pose, const double* T,
                              const int32_t* inliers, const double* inlier_rmse, const int32_t* reg_status, const double* rte,
                              const double* rre, const int32_t* success, int min_inliers, int32_t* best_rank,
                              int32_t* best_index, int32_t* reranked, double* T_rel, double* pose, int32_t* safe_pick,
                              int32_t* best_inliers, int32_t* status, double* best_rte, double* best_rre, int32_t* best_success,
                              void* stream) {
  EGONN_TRY(rel_check_shape("pick_candidates", n_queries, k, n_bank, 1));
  EGONN_REQUIRE(nn_index && map_pose && T && inliers && inlier_rmse && reg_status && best_rank && best_index && reranked && T_rel &&
                    pose && safe_pick && best_inliers && status,
                EGONN_ERR_INVALID, "pick_candidates: null pointer");
  EGONN_REQUIRE(min_inliers >= 0, EGONN_ERR_INVALID, "pick_candidates: min_inliers %d must not be negative", min_inliers);
  if (n_queries == 0) return EGONN_OK;
  hipLaunchKernelGGL(reloc_pick_kernel, dim3((unsigned)n_queries), dim3(REL_PICK_WG), 0, (hipStream_t)stream, nn_index, n_bank, k,
                     map_pose, T, inliers, inlier_rmse, reg_status, rte, rre, success, min_inliers, best_rank, best_index, reranked,
                     T_rel, pose, safe_pick, best_inliers, status, best_rte, best_rre, best_success);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
