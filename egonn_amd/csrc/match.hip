// Mutual nearest-neighbour matching of two keypoint-descriptor sets: ONE operator behind two entry points that differ only in
// how pair p finds its operands (MatchPairs below).
//
//   egonn_match_mutual      dense pairs: pair p = block p of feat1 against block p of feat2 (registration.hip consumes the result)
//   egonn_match_candidates  indexed pairs: pair p = q * k + c = (query q, map entry nn_index[q][c]), the candidate read by
//                           index from the resident bank: nothing is gathered (relocalize.hip)
//
// The rules: d2[i][j] = sum_k (a_ik - b_jk)^2 in fp64 over exactly converted fp32 descriptors, k ascending, one fma per term;
// j(i) = row argmin, i(j) = column argmin, ties: lowest index; keep (i, j(i)) with i(j(i)) == i; fewer than 3 such pairs: keep
// every (i, j(i)).  Compacted in ascending i.  d2[i][j] depends only on the order over k, so the partition over workgroups is
// free:
//   match_tile_kernel   one wave per (pair, 64 rows of side 1, 32 rows of side 2): each lane owns a row of side 1, the tile of
//                       side 2 sits in LDS, every table entry is computed ONCE; the lane's row minimum and, through an LDS
//                       transpose, the tile's column minima (rows ascending, strict <) go to scratch.
//   match_merge_kernel  per pair: partial minima merged in ascending tile order with strict < (the lowest index wins a tie, as
//                       a single ascending scan would), then the mutual filter and the compaction.
//
// No kernel reads by an unchecked index: an index outside [0, n_blocks2) yields an empty pair and a status bit.
#include "../../include/egonn_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int MATCH_TI = 64;        // rows of side 1 per workgroup of the tile kernel: one lane each, one wave
static constexpr int MATCH_TJ = 32;        // rows of side 2 per workgroup: one LDS tile
static constexpr int MATCH_WG = 256;       // lanes of the merge kernel (>= KP_MAX_N: lane t owns row t)
static constexpr int MATCH_SD_BYTES = MATCH_TJ * (MATCH_TI + 1) * 8;   // the transposed table tile

struct MatchPairs {            // pair p: side 1 = block p / k of feat1, side 2 = block (index ? index[p] : p) of feat2
  const float* feat1; const int32_t* n1;
  const float* feat2; const int32_t* n2;
  const int32_t* index;        // null: dense pairs (egonn_match_mutual), k == 1
  int k, n_blocks2;            // n_blocks2: bound of index (the map size); unused when index is null
  __device__ int block2(int p) const { return index ? index[p] : p; }
  __device__ bool valid(int b2) const { return !index || (b2 >= 0 && b2 < n_blocks2); }
};

// scratch of one call: per pair (CT + RT) * n_max slots, doubles of all pairs first, then the int32 indices in the same order.
// slot (ct, i) = row i's minimum over the columns of tile ct; slot (CT + rt, j) = column j's minimum over the rows of tile rt.
struct MatchTiles {
  int RT, CT;
  __host__ __device__ MatchTiles(int n_max) : RT((n_max + MATCH_TI - 1) / MATCH_TI), CT((n_max + MATCH_TJ - 1) / MATCH_TJ) {}
  __host__ __device__ int64_t slots(int n_max) const { return (int64_t)(RT + CT) * n_max; }
};

__global__ __launch_bounds__(MATCH_TI) void match_tile_kernel(MatchPairs mp, int n_max, int D, double* __restrict__ part_d,
                                                              int32_t* __restrict__ part_i) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_raw[];
  float4* s_tile = reinterpret_cast<float4*>(s_raw);                               // MATCH_TJ rows of D floats
  // [column of the tile][row of the tile]; it overlays the tile, which is dead once the distance loop is done: a workgroup
  // holds max(16.25 KB, 128 D bytes) of LDS instead of their sum, and twice as many waves fit a CU at D = 128
  double(*s_d)[MATCH_TI + 1] = reinterpret_cast<double(*)[MATCH_TI + 1]>(s_raw);
  const MatchTiles tl(n_max);
  const int t = threadIdx.x;
  const int ct = blockIdx.x % tl.CT, rt = (blockIdx.x / tl.CT) % tl.RT, p = blockIdx.x / (tl.CT * tl.RT);
  const int q = p / mp.k, idx = mp.block2(p);
  if (!mp.valid(idx)) return;   // (every exit before a barrier is taken by the whole workgroup)
  const int m1 = clipi(mp.n1[q], n_max), m2 = clipi(mp.n2[idx], n_max);
  const int i0 = rt * MATCH_TI, j0 = ct * MATCH_TJ;
  if (i0 >= m1 || j0 >= m2) return;   // the merge kernel reads tiles below cdiv(m1, TI) x cdiv(m2, TJ) only
  const int nrow = min(MATCH_TI, m1 - i0), ncol = min(MATCH_TJ, m2 - j0), d4 = D >> 2;
  const float4* __restrict__ own4 = reinterpret_cast<const float4*>(mp.feat1) + ((size_t)q * n_max + i0 + t) * d4;
  const float4* __restrict__ other4 = reinterpret_cast<const float4*>(mp.feat2) + ((size_t)idx * n_max + j0) * d4;
  for (int e = t; e < ncol * d4; e += MATCH_TI) s_tile[e] = other4[e];
  __syncthreads();
  double* pd = part_d + (size_t)p * tl.slots(n_max);
  int32_t* pi = part_i + (size_t)p * tl.slots(n_max);
  double acc[MATCH_TJ];
#pragma unroll
  for (int j = 0; j < MATCH_TJ; ++j) acc[j] = 0.0;
  if (t < nrow) {
    for (int kk = 0; kk < d4; ++kk) {
      const float4 a = own4[kk];
      const double ax = (double)a.x, ay = (double)a.y, az = (double)a.z, aw = (double)a.w;
#pragma unroll
      for (int j = 0; j < MATCH_TJ; ++j) {
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
  }
  __syncthreads();   // every lane is done with the tile
  if (t < nrow) {
    double best = INFINITY;
    int bj = 0;
#pragma unroll
    for (int j = 0; j < MATCH_TJ; ++j) {
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

__global__ __launch_bounds__(MATCH_WG) void match_merge_kernel(MatchPairs mp, int n_max, const double* __restrict__ part_d,
                                                               const int32_t* __restrict__ part_i, int32_t* __restrict__ corr,
                                                               int32_t* __restrict__ n_corr, int32_t* __restrict__ status) {
  __shared__ int s_j[KP_MAX_N], s_i[KP_MAX_N];
  __shared__ int s_wave[4];
  const MatchTiles tl(n_max);
  const int p = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int q = p / mp.k, idx = mp.block2(p);
  const bool valid = mp.valid(idx);
  const int m1 = valid ? clipi(mp.n1[q], n_max) : 0, m2 = valid ? clipi(mp.n2[idx], n_max) : 0;
  int32_t* out = corr + (size_t)p * n_max * 2;
  if (t == 0 && status)
    status[p] = valid ? 0 : (idx == -1 ? EGONN_RELOC_NO_CANDIDATE : (EGONN_RELOC_NO_CANDIDATE | EGONN_RELOC_BAD_INDEX));
  if (m1 == 0 || m2 == 0) {
    for (int c = t; c < n_max; c += MATCH_WG) out[2 * c] = out[2 * c + 1] = -1;
    if (t == 0) n_corr[p] = 0;
    return;
  }
  const double* pd = part_d + (size_t)p * tl.slots(n_max);
  const int32_t* pi = part_i + (size_t)p * tl.slots(n_max);
  int bj = 0, bi = 0;
  if (t < m1) {   // ascending column tiles, strict <: the lowest j of the smallest distance
    double best = INFINITY;
    const int nct = (m2 + MATCH_TJ - 1) / MATCH_TJ;
    for (int c = 0; c < nct; ++c) {
      const double v = pd[(size_t)c * n_max + t];
      if (v < best) best = v, bj = pi[(size_t)c * n_max + t];
    }
  }
  if (t < m2) {
    double best = INFINITY;
    const int nrt = (m1 + MATCH_TI - 1) / MATCH_TI;
    for (int r = 0; r < nrt; ++r) {
      const double v = pd[(size_t)(tl.CT + r) * n_max + t];
      if (v < best) best = v, bi = pi[(size_t)(tl.CT + r) * n_max + t];
    }
  }
  s_j[t] = clipi(bj, m2 - 1);   // (in range already; the clamp keeps the LDS index below in bounds whatever scratch holds)
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
  for (int c = total + t; c < n_max; c += MATCH_WG) out[2 * c] = out[2 * c + 1] = -1;
  if (t == 0) n_corr[p] = total;
}

static int64_t match_scratch_bytes(int64_t P, int n_max) { return P * MatchTiles(n_max).slots(n_max) * 12; }

// everything both entry points refuse after their shape check, in their common order, then the two launches
static int match_pairs(const char* who, const MatchPairs& mp, bool indexed, int64_t P, int n_max, int dim, int32_t* corr,
                       int32_t* n_corr, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(dim >= 4 && dim <= KP_MAX_D && dim % 4 == 0, EGONN_ERR_INVALID,
                "%s: descriptor width %d must be a multiple of 4 in [4, %d]", who, dim, KP_MAX_D);
  EGONN_REQUIRE(mp.feat1 && mp.n1 && mp.feat2 && mp.n2 && (mp.index || !indexed) && corr && n_corr && scratch, EGONN_ERR_INVALID,
                "%s: null pointer", who);
  EGONN_REQUIRE(((uintptr_t)mp.feat1 & 15) == 0 && ((uintptr_t)mp.feat2 & 15) == 0, EGONN_ERR_INVALID,
                "%s: descriptors must be 16-byte aligned", who);
  const int64_t need = match_scratch_bytes(P, n_max);
  EGONN_REQUIRE(scratch_bytes >= need && ((uintptr_t)scratch & 7) == 0, EGONN_ERR_INVALID,
                "%s: scratch needs %lld bytes, 8-byte aligned", who, (long long)need);
  if (P == 0) return EGONN_OK;
  const MatchTiles tl(n_max);
  double* part_d = (double*)scratch;
  int32_t* part_i = (int32_t*)(part_d + P * tl.slots(n_max));
  const size_t lds = std::max((size_t)MATCH_SD_BYTES, (size_t)MATCH_TJ * dim * sizeof(float));   // 16.25-32 KB
  hipLaunchKernelGGL(match_tile_kernel, dim3((unsigned)(P * tl.RT * tl.CT)), dim3(MATCH_TI), lds, (hipStream_t)stream, mp, n_max,
                     dim, part_d, part_i);
  HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned)P), dim3(MATCH_WG), 0, (hipStream_t)stream, mp, n_max, part_d, part_i, corr,
                     n_corr, status);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace egonn

using namespace egonn;

API int64_t egonn_match_mutual_scratch_bytes(int n_pairs, int n_max) {
  if (n_pairs < 0 || n_pairs > KP_MAX_PAIRS || n_max < 1 || n_max > KP_MAX_N) return -1;
  return match_scratch_bytes(n_pairs, n_max);
}

API int egonn_match_mutual(const float* feat1, const float* feat2, const int32_t* n1, const int32_t* n2, int n_pairs, int n_max,
                           int dim, int32_t* corr, int32_t* n_corr, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_TRY(reg_check_shape("match_mutual", n_pairs, n_max));
  const MatchPairs mp = {feat1, n1, feat2, n2, nullptr, 1, 0};
  return match_pairs("match_mutual", mp, false, n_pairs, n_max, dim, corr, n_corr, nullptr, scratch, scratch_bytes, stream);
}

API int64_t egonn_match_candidates_scratch_bytes(int n_queries, int k, int n_max) {
  if (n_queries < 0 || k < 1 || k > REL_MAX_K || (int64_t)n_queries * k > KP_MAX_PAIRS || n_max < 1 || n_max > KP_MAX_N) return -1;
  return match_scratch_bytes((int64_t)n_queries * k, n_max);
}

API int egonn_match_candidates(const float* q_feat, const int32_t* q_n, const float* bank_feat, const int32_t* bank_n,
                               const int32_t* nn_index, int n_queries, int k, int n_bank, int n_max, int dim, int32_t* corr,
                               int32_t* n_corr, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_TRY(rel_check_shape("match_candidates", n_queries, k, n_bank, n_max));
  const MatchPairs mp = {q_feat, q_n, bank_feat, bank_n, nn_index, k, n_bank};
  return match_pairs("match_candidates", mp, true, (int64_t)n_queries * k, n_max, dim, corr, n_corr, status,
                     scratch, scratch_bytes, stream);
}
