// Relocalisation of query scans against a resident keypoint map: the top-k candidates of the global retrieval are verified
// by keypoint registration and the one with the most inliers gives the 6-DoF pose (P_query = P_map[best] @ T, with T the
// transform of registration.hip that maps query keypoints into the candidate's frame; misc/poses.py: T_gt = inv(P_map) @ P_query).
//
//   1. egonn_match_candidates  mutual nearest-neighbour matching of pair p = q * k + c = (query q, map entry nn_index[q][c]),
//                              the candidate read by index from the bank: nothing is gathered.  The rules and every bit are
//                              those of reg_match_kernel (registration.hip): d2[i][j] = sum_k (a_ik - b_jk)^2 in fp64 over
//                              exactly converted fp32 inputs, k ascending, one fma per term.  d2[i][j] depends only on the
//                              order over k, so the partition over workgroups is free:
//        reloc_tile_kernel     one wave per (pair, 64 query rows, 32 candidate rows): each lane owns a query row, the
//                              candidate tile sits in LDS, every table entry is computed ONCE; the lane's row minimum and,
//                              through an LDS transpose, the tile's column minima (rows ascending, strict <) go to scratch.
//        reloc_merge_kernel    per pair: partial minima merged in ascending tile order with strict < (the lowest index wins a
//                              tie, as a single ascending scan would), then the mutual filter and the compaction, word for
//                              word the tail of reg_match_kernel.
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

static constexpr int REL_MAX_N = 256;    // keypoints per side, as registration.hip
static constexpr int REL_MAX_D = 256;    // descriptor width
static constexpr int REL_TI = 64;        // query rows per workgroup of the tile kernel: one lane each, one wave
static constexpr int REL_TJ = 32;        // candidate rows per workgroup: one LDS tile
static constexpr int REL_WG = 256;       // lanes of the merge and gather kernels (>= REL_MAX_N: lane t owns row t)
static constexpr int REL_PICK_WG = 64;
static constexpr int REL_MAX_K = 1024;   // candidates per query
static constexpr int REL_SD_BYTES = REL_TJ * (REL_TI + 1) * 8;   // the transposed table tile; a multiple of 16

__device__ static inline int rel_clip(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// scratch of one call: per pair (CT + RT) * n_max slots, doubles of all pairs first, then the int32 indices in the same order.
// slot (ct, i) = row i's minimum over the columns of tile ct; slot (CT + rt, j) = column j's minimum over the rows of tile rt.
struct RelTiles {
  int RT, CT;
  __host__ __device__ RelTiles(int n_max) : RT((n_max + REL_TI - 1) / REL_TI), CT((n_max + REL_TJ - 1) / REL_TJ) {}
  __host__ __device__ int64_t slots(int n_max) const { return (int64_t)(RT + CT) * n_max; }
};

__global__ __launch_bounds__(REL_TI) void reloc_tile_kernel(const float* __restrict__ q_feat, const int32_t* __restrict__ q_n,
                                                           const float* __restrict__ bank_feat,
                                                           const int32_t* __restrict__ bank_n,
                                                           const int32_t* __restrict__ nn_index, int M, int k, int n_max, int D,
                                                           double* __restrict__ part_d, int32_t* __restrict__ part_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  double(*s_d)[REL_TI + 1] = reinterpret_cast<double(*)[REL_TI + 1]>(s_raw);   // [column of the tile][row of the tile]
  float4* s_tile = reinterpret_cast<float4*>(s_raw + REL_SD_BYTES);            // REL_TJ rows of D floats
  const RelTiles tl(n_max);
  const int t = threadIdx.x;
  const int ct = blockIdx.x % tl.CT, rt = (blockIdx.x / tl.CT) % tl.RT, p = blockIdx.x / (tl.CT * tl.RT);
  const int q = p / k, idx = nn_index[p];
  if (idx < 0 || idx >= M) return;   // (every exit before a barrier is taken by the whole workgroup)
  const int m1 = rel_clip(q_n[q], n_max), m2 = rel_clip(bank_n[idx], n_max);
  const int i0 = rt * REL_TI, j0 = ct * REL_TJ;
  if (i0 >= m1 || j0 >= m2) return;   // the merge kernel reads tiles below cdiv(m1, TI) x cdiv(m2, TJ) only
  const int nrow = min(REL_TI, m1 - i0), ncol = min(REL_TJ, m2 - j0), d4 = D >> 2;
  const float4* own4 = reinterpret_cast<const float4*>(q_feat) + ((size_t)q * n_max + i0 + t) * d4;
  const float4* other4 = reinterpret_cast<const float4*>(bank_feat) + ((size_t)idx * n_max + j0) * d4;
  for (int e = t; e < ncol * d4; e += REL_TI) s_tile[e] = other4[e];
  __syncthreads();
  double* pd = part_d + (size_t)p * tl.slots(n_max);
  int32_t* pi = part_i + (size_t)p * tl.slots(n_max);
  if (t < nrow) {
    double acc[REL_TJ];
#pragma unroll
    for (int j = 0; j < REL_TJ; ++j) acc[j] = 0.0;
    for (int kk = 0; kk < d4; ++kk) {
      const float4 a = own4[kk];
      const double ax = (double)a.x, ay = (double)a.y, az = (double)a.z, aw = (double)a.w;
#pragma unroll
      for (int j = 0; j < REL_TJ; ++j) {
        const float4 b = s_tile[j * d4 + kk];   // rows >= ncol hold stale data: computed, never compared
        double d = ax - (double)b.x;
        acc[j] = fma(d, d, acc[j]);
        d = ay - (double)b.y;
        acc[j] = fma(d, d, acc[j]);
        d = az - (double)b.z;
        acc[j] = fma(d, d, acc[j]);
        d = aw - (double)b.w;
        acc[j] = fma(d, d, acc[j]);
      }
    }
    double best = INFINITY;
    int bj = 0;
#pragma unroll
    for (int j = 0; j < REL_TJ; ++j) {
      s_d[j][t] = acc[j];
      if (j < ncol && acc[j] < best) {
        best = acc[j];
        bj = j0 + j;
      }
    }
    pd[(size_t)ct * n_max + i0 + t] = best;
    pi[(size_t)ct * n_max + i0 + t] = bj;
  }
  __syncthreads();
  if (t < ncol) {   // lane t: column t of the tile, rows ascending (stride 65 doubles: no bank conflict)
    double best = INFINITY;
    int bi = 0;
    for (int r = 0; r < nrow; ++r) {
      const double v = s_d[t][r];
      if (v < best) {
        best = v;
        bi = i0 + r;
      }
    }
    pd[(size_t)(tl.CT + rt) * n_max + j0 + t] = best;
    pi[(size_t)(tl.CT + rt) * n_max + j0 + t] = bi;
  }
}

__global__ __launch_bounds__(REL_WG) void reloc_merge_kernel(const int32_t* __restrict__ q_n, const int32_t* __restrict__ bank_n,
                                                             const int32_t* __restrict__ nn_index, int M, int k, int n_max,
                                                             const double* __restrict__ part_d,
                                                             const int32_t* __restrict__ part_i, int32_t* __restrict__ corr,
                                                             int32_t* __restrict__ n_corr, int32_t* __restrict__ status) {
  __shared__ int s_j[REL_MAX_N], s_i[REL_MAX_N];
  __shared__ int s_wave[4];
  const RelTiles tl(n_max);
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int q = p / k, idx = nn_index[p];
  const bool valid = idx >= 0 && idx < M;
  const int m1 = valid ? rel_clip(q_n[q], n_max) : 0, m2 = valid ? rel_clip(bank_n[idx], n_max) : 0;
  int32_t* out = corr + (size_t)p * n_max * 2;
  if (t == 0 && status)
    status[p] = valid ? 0 : (idx == -1 ? EGONN_RELOC_NO_CANDIDATE : (EGONN_RELOC_NO_CANDIDATE | EGONN_RELOC_BAD_INDEX));
  if (m1 == 0 || m2 == 0) {
    for (int c = t; c < n_max; c += REL_WG) out[2 * c] = out[2 * c + 1] = -1;
    if (t == 0) n_corr[p] = 0;
    return;
  }
  const double* pd = part_d + (size_t)p * tl.slots(n_max);
  const int32_t* pi = part_i + (size_t)p * tl.slots(n_max);
  int bj = 0, bi = 0;
  if (t < m1) {   // ascending column tiles, strict <: the lowest j of the smallest distance
    double best = INFINITY;
    const int nct = (m2 + REL_TJ - 1) / REL_TJ;
    for (int c = 0; c < nct; ++c) {
      const double v = pd[(size_t)c * n_max + t];
      if (v < best) best = v, bj = pi[(size_t)c * n_max + t];
    }
  }
  if (t < m2) {
    double best = INFINITY;
    const int nrt = (m1 + REL_TI - 1) / REL_TI;
    for (int r = 0; r < nrt; ++r) {
      const double v = pd[(size_t)(tl.CT + r) * n_max + t];
      if (v < best) best = v, bi = pi[(size_t)(tl.CT + r) * n_max + t];
    }
  }
  s_j[t] = rel_clip(bj, m2 - 1);   // (in range already; the clamp keeps the LDS index below in bounds whatever scratch holds)
  s_i[t] = bi;
  __syncthreads();
  const bool mutual = t < m1 && s_i[s_j[t]] == t;
  unsigned long long bal = __ballot(mutual);
  if (lane == 0) s_wave[w] = __popcll(bal);
  __syncthreads();
  const int n_mutual = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  __syncthreads();
  const bool keep = n_mutual >= 3 ? mutual : (t < m1);
  bal = __ballot(keep);
  if (lane == 0) s_wave[w] = __popcll(bal);
  __syncthreads();
  int pos = __popcll(bal & ((1ull << lane) - 1ull));
  for (int c = 0; c < w; ++c) pos += s_wave[c];
  const int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
  if (keep) {
    out[2 * pos] = t;
    out[2 * pos + 1] = s_j[t];
  }
  for (int c = total + t; c < n_max; c += REL_WG) out[2 * c] = out[2 * c + 1] = -1;
  if (t == 0) n_corr[p] = total;
}

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
  safe_pick[q] = ok ? idx : rel_clip(head, M - 1);
  best_inliers[q] = ok ? inliers[base + first] : 0;
  status[q] = bits | (ok ? 0 : EGONN_RELOC_UNVERIFIED);
  if (best_rte) best_rte[q] = ok && rte ? rte[base + first] : -1.0;
  if (best_rre) best_rre[q] = ok && rre ? rre[base + first] : -1.0;
  if (best_success) best_success[q] = ok && success ? success[base + first] : 0;
}

static int rel_check_shape(const char* who, int Q, int k, int M, int n_max) {
  EGONN_REQUIRE(Q >= 0 && k >= 1 && k <= REL_MAX_K && (int64_t)Q * k <= (1 << 20), EGONN_ERR_INVALID,
                "%s: bad shape (n_queries=%d, k=%d; 1 <= k <= %d, n_queries * k <= 2^20)", who, Q, k, REL_MAX_K);
  EGONN_REQUIRE(M >= 1, EGONN_ERR_INVALID, "%s: the map needs at least one entry (n_bank=%d)", who, M);
  EGONN_REQUIRE(n_max >= 1 && n_max <= REL_MAX_N, EGONN_ERR_INVALID, "%s: bad shape (n_max=%d; 1 <= n_max <= %d)", who, n_max,
                REL_MAX_N);
  return EGONN_OK;
}

}  // namespace egonn

using namespace egonn;

API int64_t egonn_match_candidates_scratch_bytes(int n_queries, int k, int n_max) {
  if (n_queries < 0 || k < 1 || k > REL_MAX_K || (int64_t)n_queries * k > (1 << 20) || n_max < 1 || n_max > REL_MAX_N) return -1;
  return (int64_t)n_queries * k * RelTiles(n_max).slots(n_max) * 12;
}

API int egonn_match_candidates(const float* q_feat, const int32_t* q_n, const float* bank_feat, const int32_t* bank_n,
                               const int32_t* nn_index, int n_queries, int k, int n_bank, int n_max, int dim, int32_t* corr,
                               int32_t* n_corr, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_TRY(rel_check_shape("match_candidates", n_queries, k, n_bank, n_max));
  EGONN_REQUIRE(dim >= 4 && dim <= REL_MAX_D && dim % 4 == 0, EGONN_ERR_INVALID,
                "match_candidates: descriptor width %d must be a multiple of 4 in [4, %d]", dim, REL_MAX_D);
  EGONN_REQUIRE(q_feat && q_n && bank_feat && bank_n && nn_index && corr && n_corr && scratch, EGONN_ERR_INVALID,
                "match_candidates: null pointer");
  EGONN_REQUIRE(((uintptr_t)q_feat & 15) == 0 && ((uintptr_t)bank_feat & 15) == 0, EGONN_ERR_INVALID,
                "match_candidates: descriptors must be 16-byte aligned");
  const int64_t need = egonn_match_candidates_scratch_bytes(n_queries, k, n_max);
  EGONN_REQUIRE(scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0, EGONN_ERR_INVALID,
                "match_candidates: scratch needs %lld bytes, 8-byte aligned", (long long)need);
  if (n_queries == 0) return EGONN_OK;
  const int64_t P = (int64_t)n_queries * k;
  const RelTiles tl(n_max);
  double* part_d = (double*)scratch;
  int32_t* part_i = (int32_t*)(part_d + P * tl.slots(n_max));
  const size_t lds = (size_t)REL_SD_BYTES + (size_t)REL_TJ * dim * sizeof(float);   // <= 48.25 KB: below the 64 KB default limit
  hipLaunchKernelGGL(reloc_tile_kernel, dim3((unsigned)(P * tl.RT * tl.CT)), dim3(REL_TI), lds, (hipStream_t)stream, q_feat, q_n,
                     bank_feat, bank_n, nn_index, n_bank, k, n_max, dim, part_d, part_i);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(reloc_merge_kernel, dim3((unsigned)P), dim3(REL_WG), 0, (hipStream_t)stream, q_n, bank_n, nn_index, n_bank, k,
                     n_max, part_d, part_i, corr, n_corr, status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

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
