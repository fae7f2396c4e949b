// Training augmentation of a resident scan batch on the device — the stage in front of egonn_voxelize_device.  It restates
// datasets/augmentation.py as the reference configures it, at its three call sites, in the reference's order:
//
//   stage 1, per scan (TrainTransform, datasets/base_datasets.py:70-76)
//     JitterPoints(sigma, clip), p = 1   j = clamp(fp32(sigma) * fp32(normal), -clip, clip);  point = point + j        (fp32)
//     RemoveRandomPoints(r)              r = r_min + (r_max - r_min) * u;  k = int(n * r) in fp64;  exactly k distinct points
//                                        are set to (0, 0, 0) — zeroed, not dropped, and moved by what follows
//     RandomTranslation(max_delta)       t = fp32(max_delta * normal) per axis, one per scan;  point = point + t
//     RandomRotation(max_theta, z)       theta = ((pi * max_theta) / 180 * 2) * (u - 0.5);  c, s = fp32(cos), fp32(sin);
//                                        coords @ R:  x' = x*c + y*s,  y' = x*(-s) + y*c                              (mode 2)
//     RemoveRandomBlock(p, scale, ratio) with u < p: a cuboid from the CURRENT fp32 bounding box (removed points included),
//                                        strict comparisons, points inside set to zero (aug_param_kernel)
//   stage 2, per batch (TrainSetTransform, datasets/dataset_utils.py:67-72), one draw for all scans
//     RandomRotation(max_theta, z)       as above                                                                     (mode 1)
//     RandomFlip(p)                      u <= cum[0]: x = -x;  else u <= cum[1]: y = -y;  else u <= cum[2]: z = -z
//   stage 3, per scan (datasets/mulran/mulran_train.py:41-50)
//     angle = -rot_max + (2 rot_max) * u;  m = [[c, s, 0, tx], [-s, c, 0, ty], [0, 0, 1, 0], [0, 0, 0, 1]] in fp32 with
//     tx, ty = (u24 * 2) * trans_max - trans_max in fp32;  point = pc @ m[:3,:3].T + m[:3,3] (misc/poses.py:68-76);
//     T_out = m @ T_in in fp32 (k ascending, no fma)
//
// Deliberate differences from the reference: (a) its generators (Python's, NumPy's and torch's global streams) are
// replaced by the counter-based draw below, so a scan's augmentation does not depend on the batch it sits in, on its
// position there, or on eager / replayed execution, and the host can reproduce it; (b) the removed set is the k smallest
// of the per-point keys, a uniformly random k-subset like np.random.choice(replace=False), not NumPy's permutation; (c) an
// empty scan draws no block (the reference's torch.min raises on it); (d) 3-term sums run in ascending order (BLAS's order
// is its own).  max_theta2, random axes, JitterPoints(p < 1), RandomScale and RandomShear are not configured anywhere in
// the reference and are refused by the Python layer.
//
// The draw.  With 64-bit wrapping arithmetic
//       ctr = (draw << 50) | (id << 28) | (point << 4) | slot      draw < 2^14, id < 2^22, point < 2^24, slot < 2^4
//       z   = seed + 0x9E3779B97F4A7C15 * (ctr + 1)                (the state of splitmix64(seed) after ctr + 1 steps)
//       z   = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9
//       z   = (z ^ (z >> 27)) * 0x94D049BB133111EB
//       z   =  z ^ (z >> 31)
//   uniform  u   = (z >> 11) * 2^-53                               fp64, in [0, 1)
//   uniform  u24 = fp32(z >> 40) * 2^-24                           fp32, in [0, 1), exact
//   normal   g   = sqrt(-2 * log(((z >> 32) + 1) * 2^-32)) * cos(6.283185307179586 * ((z & 0xFFFFFFFF) * 2^-32))
//                  in fp64, every operation as written, rounded ONCE to fp32 where the reference's generator is fp32
//   per point  (point = index inside the scan, < 2^24 - 2; id = the caller's scan id):
//       slot 0, 1, 2: jitter normal of x, y, z;  slot 3: removal key = (z & ~0xFFFFFF) | point  (unique per scan)
//   per scan   (point = 0xFFFFFF; id = the caller's scan id):
//       slot 0: r;  1, 2, 3: translation normals;  4: rotation u;  5: block u;  6: area u;  7: aspect u;  8: x u;  9: y u;
//       slot 10: rigid angle u;  11, 12: rigid tx, ty u24
//   per batch  (point = 0xFFFFFE; id = set_id):  slot 0: set rotation u;  1: flip u
// Fields that do not fit fail loudly: draw, set_id and the capacity n on the host (EGONN_STATUS_INVALID); a scan id outside
// [0, 2^22) on the device: status bit EGONN_AUG_STATUS_BAD_ID in the record and NaN in every point of that scan.
//
// Launches: aug_select_kernel (one workgroup per scan: the per-scan draws and a compute-only radix select of the k-th
// smallest key, 8 passes of 8 bits, histograms in LDS), aug_box_kernel (AUG_CHUNKS workgroups per scan recompute the point
// and reduce min / max, which are exact, so any order gives the same bits), aug_param_kernel (block, set and records) and
// aug_apply_kernel (one point per lane: recompute, erase, set transform, rigid after-stage, store).  No float atomics, no
// host synchronisation; counts and offsets are read on the device, rows beyond scan_offsets[batch_size] are untouched.
#include "../../include/egonn_hip.h"
#include "common.h"

#pragma clang fp contract(off)

namespace egonn {

static constexpr int AUG_TILE = 256;        // points per workgroup of the apply pass (one per lane)
static constexpr int AUG_SEL_WG = 1024;     // lanes of the per-scan select workgroup
static constexpr int AUG_CHUNKS = 16;       // workgroups per scan of the bounding-box pass
static constexpr int AUG_BOX_WG = 256;
static constexpr uint32_t AUG_PT_SCAN = 0xFFFFFFu, AUG_PT_SET = 0xFFFFFEu;
static constexpr int AUG_REC_I = 8, AUG_REC_D = 32;

struct AugScan {
  uint64_t thresh;      // removed iff key <= thresh (k > 0)
  int64_t lo;
  int32_t n, k, block_on, status;
  uint32_t id;
  float t[3];           // RandomTranslation
  float c1, s1;         // RandomRotation (stage 1)
  float bx0, bx1, by0, by1;
  float m[12];          // rigid after-stage, rows of the 3 x 4
};
struct AugSet {
  float c, s;
  int32_t flip;         // axis, -1 = none
  int32_t pad;
};

__host__ __device__ static inline uint64_t aug_hash(uint64_t seed, uint32_t draw, uint32_t id, uint32_t point, uint32_t slot) {
  const uint64_t ctr = ((uint64_t)draw << 50) | ((uint64_t)id << 28) | ((uint64_t)point << 4) | (uint64_t)slot;
  uint64_t z = seed + 0x9E3779B97F4A7C15ull * (ctr + 1ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__device__ static inline double aug_uniform(uint64_t z) { return (double)(z >> 11) * 0x1p-53; }
__device__ static inline float aug_uniform24(uint64_t z) { return (float)(uint32_t)(z >> 40) * 0x1p-24f; }
__device__ static inline double aug_normal(uint64_t z) {
  const double u1 = ((double)(z >> 32) + 1.0) * 0x1p-32, u2 = (double)(z & 0xFFFFFFFFull) * 0x1p-32;
  return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}
__device__ static inline uint64_t aug_key(const egonn_augment_params& c, uint32_t id, uint32_t i) {
  return (aug_hash(c.seed, c.draw, id, i, 3) & ~0xFFFFFFull) | (uint64_t)i;
}
__device__ static inline double aug_theta(double max_theta, double u) {
  return ((3.141592653589793 * max_theta) / 180.0) * 2.0 * (u - 0.5);
}

// rows [lo, lo + len) of scan b, clamped into [0, min(n, offsets[B])] so that nothing is indexed by an unchecked offset
__device__ static inline void aug_range(const int64_t* __restrict__ off, int b, int B, int64_t n, int64_t& lo, int64_t& len) {
  const int64_t end = max((int64_t)0, min(n, off[B]));
  lo = max((int64_t)0, min(end, off[b]));
  const int64_t hi = max(lo, min(end, off[b + 1]));
  len = hi - lo;
}

// stage 1 of one point up to and including the rotation: what the bounding box of RemoveRandomBlock sees
__device__ static inline bool aug_stage1(const egonn_augment_params& c, const AugScan& S, uint32_t i, float& x, float& y,
                                         float& z) {
  if (c.stages & EGONN_AUG_JITTER) {
    const float sg = (float)c.sigma, cl = (float)c.clip;
    float j[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      j[a] = sg * (float)aug_normal(aug_hash(c.seed, c.draw, S.id, i, a));
      if (c.stages & EGONN_AUG_JITTER_CLIP) j[a] = fminf(fmaxf(j[a], -cl), cl);
    }
    x = x + j[0];
    y = y + j[1];
    z = z + j[2];
  }
  const bool removed = S.k > 0 && aug_key(c, S.id, i) <= S.thresh;
  if (removed) x = y = z = 0.f;
  if (c.stages & EGONN_AUG_TRANSLATE) {
    x = x + S.t[0];
    y = y + S.t[1];
    z = z + S.t[2];
  }
  if (c.stages & EGONN_AUG_ROTATE) {
    const float nx = x * S.c1 + y * S.s1, ny = x * (-S.s1) + y * S.c1;
    x = nx;
    y = ny;
  }
  return removed;
}

// ------------------------------------------------------------------ 1. per-scan draws and the removal threshold
__global__ __launch_bounds__(AUG_SEL_WG) void aug_select_kernel(const int64_t* __restrict__ off, int B, int64_t n,
                                                                const int32_t* __restrict__ scan_ids,
                                                                egonn_augment_params c, AugScan* __restrict__ scans) {
  __shared__ uint32_t s_hist[256];
  __shared__ uint32_t s_digit, s_rem;
  const int b = blockIdx.x, t = threadIdx.x;
  int64_t lo, len64;
  aug_range(off, b, B, n, lo, len64);
  const uint32_t len = (uint32_t)len64;                 // n < 2^24 on the host
  const int64_t raw_id = scan_ids ? (int64_t)scan_ids[b] : (int64_t)b;
  const bool bad = raw_id < 0 || raw_id >= (1ll << 22) || len >= AUG_PT_SET;
  const uint32_t id = bad ? 0u : (uint32_t)raw_id;
  double r = 0.0;
  uint32_t k = 0;
  if (c.stages & EGONN_AUG_REMOVE_POINTS) {
    r = c.r_min + (c.r_max - c.r_min) * aug_uniform(aug_hash(c.seed, c.draw, id, AUG_PT_SCAN, 0));
    const double kd = (double)len * r;
    k = kd > 0.0 ? (kd >= (double)len ? len : (uint32_t)kd) : 0u;     // int(n * r), kept inside [0, n]
  }
  uint64_t prefix = 0;
  if (k > 0) {
    uint32_t rem = k;
    for (int pass = 7; pass >= 0; --pass) {
      const int shift = pass * 8;
      const uint64_t hi_mask = pass == 7 ? 0ull : (~0ull << (shift + 8));
      if (t < 256) s_hist[t] = 0;
      __syncthreads();
      for (uint32_t i = t; i < len; i += AUG_SEL_WG) {
        const uint64_t key = aug_key(c, id, i);
        if ((key & hi_mask) == prefix) atomicAdd(&s_hist[(uint32_t)(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      if (t == 0) {
        uint32_t cum = 0;
        int d = 0;
        for (; d < 255; ++d) {
          if (cum + s_hist[d] >= rem) break;
          cum += s_hist[d];
        }
        s_digit = (uint32_t)d;
        s_rem = rem - cum;
      }
      __syncthreads();
      prefix |= (uint64_t)s_digit << shift;
      rem = s_rem;
      __syncthreads();
    }
  }
  if (t == 0) {
    AugScan S;
    S.thresh = prefix;
    S.lo = lo;
    S.n = (int32_t)len;
    S.k = (int32_t)k;
    S.block_on = 0;
    S.status = bad ? EGONN_AUG_STATUS_BAD_ID : 0;
    S.id = id;
    S.t[0] = S.t[1] = S.t[2] = 0.f;
    if (c.stages & EGONN_AUG_TRANSLATE)
      for (int a = 0; a < 3; ++a)
        S.t[a] = (float)(c.max_delta * aug_normal(aug_hash(c.seed, c.draw, id, AUG_PT_SCAN, 1 + a)));
    S.c1 = 1.f;
    S.s1 = 0.f;
    if (c.stages & EGONN_AUG_ROTATE) {
      const double th = aug_theta(c.max_theta, aug_uniform(aug_hash(c.seed, c.draw, id, AUG_PT_SCAN, 4)));
      S.c1 = (float)cos(th);
      S.s1 = (float)sin(th);
    }
    S.bx0 = S.bx1 = S.by0 = S.by1 = 0.f;
    for (int a = 0; a < 12; ++a) S.m[a] = (a == 0 || a == 5 || a == 10) ? 1.f : 0.f;
    scans[b] = S;
  }
}

// ------------------------------------------------------------------ 2. bounding box of the moved points
__global__ __launch_bounds__(AUG_BOX_WG) void aug_box_kernel(const float* __restrict__ pts, const int64_t* __restrict__ off,
                                                             int B, int64_t n, egonn_augment_params c,
                                                             const AugScan* __restrict__ scans, float* __restrict__ partial) {
  __shared__ float s_red[AUG_BOX_WG / 64][6];
  const int ch = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const AugScan S = scans[b];
  const int64_t len = S.n;
  const int64_t i0 = len * ch / AUG_CHUNKS, i1 = len * (ch + 1) / AUG_CHUNKS;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = i0 + t; i < i1; i += AUG_BOX_WG) {
    const float* p = pts + (S.lo + i) * 3;
    float x = p[0], y = p[1], z = p[2];
    aug_stage1(c, S, (uint32_t)i, x, y, z);
    mn[0] = fminf(mn[0], x);
    mn[1] = fminf(mn[1], y);
    mn[2] = fminf(mn[2], z);
    mx[0] = fmaxf(mx[0], x);
    mx[1] = fmaxf(mx[1], y);
    mx[2] = fmaxf(mx[2], z);
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    for (int o = 32; o >= 1; o >>= 1) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], o, 64));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o, 64));
    }
  if ((t & 63) == 0)
    for (int a = 0; a < 3; ++a) {
      s_red[t >> 6][a] = mn[a];
      s_red[t >> 6][3 + a] = mx[a];
    }
  __syncthreads();
  if (t < 6) {
    float v = s_red[0][t];
    for (int w = 1; w < AUG_BOX_WG / 64; ++w) v = t < 3 ? fminf(v, s_red[w][t]) : fmaxf(v, s_red[w][t]);
    partial[((size_t)b * AUG_CHUNKS + ch) * 6 + t] = v;
  }
}

// ------------------------------------------------------------------ 3. block, set and rigid parameters, records
__global__ __launch_bounds__(64) void aug_param_kernel(int B, egonn_augment_params c, AugScan* __restrict__ scans,
                                                       AugSet* __restrict__ set, const float* __restrict__ partial,
                                                       const float* __restrict__ T_in, float* __restrict__ T_out,
                                                       int32_t* __restrict__ rec_i, double* __restrict__ rec_d) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  // the batch's draw: computed by every lane (a pure function), stored by one
  double th_set = 0.0, u_flip = 0.0;
  AugSet Q;
  Q.c = 1.f;
  Q.s = 0.f;
  Q.flip = -1;
  Q.pad = 0;
  if (c.stages & EGONN_AUG_SET_ROTATE) {
    th_set = aug_theta(c.set_max_theta, aug_uniform(aug_hash(c.seed, c.draw, c.set_id, AUG_PT_SET, 0)));
    Q.c = (float)cos(th_set);
    Q.s = (float)sin(th_set);
  }
  if (c.stages & EGONN_AUG_FLIP) {
    u_flip = aug_uniform(aug_hash(c.seed, c.draw, c.set_id, AUG_PT_SET, 1));
    Q.flip = u_flip <= c.flip_cum[0] ? 0 : (u_flip <= c.flip_cum[1] ? 1 : (u_flip <= c.flip_cum[2] ? 2 : -1));
  }
  if (b == 0) *set = Q;
  if (b >= B) return;
  AugScan S = scans[b];
  double d[AUG_REC_D];
  for (int a = 0; a < AUG_REC_D; ++a) d[a] = 0.0;
  if (c.stages & EGONN_AUG_REMOVE_POINTS)
    d[0] = c.r_min + (c.r_max - c.r_min) * aug_uniform(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 0));
  if (c.stages & EGONN_AUG_TRANSLATE)
    for (int a = 0; a < 3; ++a) d[1 + a] = c.max_delta * aug_normal(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 1 + a));
  if (c.stages & EGONN_AUG_ROTATE) {
    d[4] = aug_theta(c.max_theta, aug_uniform(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 4)));
    d[5] = cos(d[4]);
    d[6] = sin(d[4]);
  }
  if (c.stages & EGONN_AUG_BLOCK) {
    const double ub = aug_uniform(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 5));
    d[7] = ub;
    float bb[6];
    for (int a = 0; a < 6; ++a) {
      float v = partial[(size_t)b * AUG_CHUNKS * 6 + a];
      for (int ch = 1; ch < AUG_CHUNKS; ++ch) {
        const float w = partial[((size_t)b * AUG_CHUNKS + ch) * 6 + a];
        v = a < 3 ? fminf(v, w) : fmaxf(v, w);
      }
      bb[a] = v;
      d[8 + a] = (double)v;
    }
    if (ub < c.block_p && S.n > 0) {
      // get_params: the box is an fp32 tensor, Python's scalars are rounded to fp32 where they meet it, math.sqrt is fp64
      const float span0 = bb[3] - bb[0], span1 = bb[4] - bb[1];
      const float area = span0 * span1;
      const double ua = c.scale_lo + (c.scale_hi - c.scale_lo) * aug_uniform(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 6));
      const double ar = c.ratio_lo + (c.ratio_hi - c.ratio_lo) * aug_uniform(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 7));
      const float ea = (float)ua * area;
      const double h = sqrt((double)(ea * (float)ar)), w = sqrt((double)(ea / (float)ar));
      const double ux = 0.0 + (1.0 - 0.0) * aug_uniform(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 8));
      const double uy = 0.0 + (1.0 - 0.0) * aug_uniform(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 9));
      S.bx0 = bb[0] + (float)ux * (span0 - (float)w);
      S.by0 = bb[1] + (float)uy * (span1 - (float)h);
      S.bx1 = S.bx0 + (float)w;
      S.by1 = S.by0 + (float)h;
      S.block_on = 1;
      d[14] = (double)S.bx0;
      d[15] = (double)S.by0;
      d[16] = w;
      d[17] = h;
      d[18] = (double)S.bx1;
      d[19] = (double)S.by1;
      d[29] = (double)ea;
      d[30] = ar;
    }
  }
  d[20] = th_set;
  d[21] = (c.stages & EGONN_AUG_SET_ROTATE) ? cos(th_set) : 0.0;
  d[22] = (c.stages & EGONN_AUG_SET_ROTATE) ? sin(th_set) : 0.0;
  d[23] = u_flip;
  if (c.stages & EGONN_AUG_RIGID) {
    const double ang = -c.rot_max + (c.rot_max - (-c.rot_max)) * aug_uniform(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 10));
    const float cv = (float)cos(ang), sv = (float)sin(ang), tm = (float)c.trans_max;
    const float tx = aug_uniform24(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 11)) * 2.f * tm - tm;
    const float ty = aug_uniform24(aug_hash(c.seed, c.draw, S.id, AUG_PT_SCAN, 12)) * 2.f * tm - tm;
    S.m[0] = cv;
    S.m[1] = sv;
    S.m[3] = tx;
    S.m[4] = -sv;
    S.m[5] = cv;
    S.m[7] = ty;
    d[24] = ang;
    d[25] = cos(ang);
    d[26] = sin(ang);
    d[27] = (double)tx;
    d[28] = (double)ty;
  }
  if (T_out) {
    for (int r = 0; r < 4; ++r)
      for (int q = 0; q < 4; ++q) {
        float acc = 0.f;
        for (int k = 0; k < 4; ++k) {
          const float mk = r < 3 ? S.m[r * 4 + k] : (k == 3 ? 1.f : 0.f);
          const float tk = T_in ? T_in[(size_t)b * 16 + k * 4 + q] : (k == q ? 1.f : 0.f);
          acc = acc + mk * tk;
        }
        T_out[(size_t)b * 16 + r * 4 + q] = acc;
      }
  }
  scans[b] = S;
  if (rec_i) {
    int32_t* ri = rec_i + (size_t)b * AUG_REC_I;
    ri[0] = S.n;
    ri[1] = S.k;
    ri[2] = S.block_on;
    ri[3] = Q.flip;
    ri[4] = S.status;
    ri[5] = (int32_t)S.id;
    ri[6] = (int32_t)(uint32_t)(S.thresh & 0xFFFFFFFFull);
    ri[7] = (int32_t)(uint32_t)(S.thresh >> 32);
  }
  if (rec_d)
    for (int a = 0; a < AUG_REC_D; ++a) rec_d[(size_t)b * AUG_REC_D + a] = d[a];
}

// ------------------------------------------------------------------ 4. recompute, erase, set transform, after-stage, store
// pts and out may be one array (a lane reads its own row before it writes it), so neither is __restrict__
__global__ __launch_bounds__(AUG_TILE) void aug_apply_kernel(const float* pts, const int64_t* __restrict__ off, int B, int64_t n,
                                                             egonn_augment_params c, const AugScan* __restrict__ scans,
                                                             const AugSet* __restrict__ set, float* out,
                                                             uint8_t* __restrict__ flags) {
  const int64_t row = (int64_t)blockIdx.x * AUG_TILE + threadIdx.x;
  const int64_t end = max((int64_t)0, min(n, off[B]));
  if (row >= end) return;                      // rows beyond the live count are untouched
  int lo = 0, hi = B;                          // the last scan b in [0, B) whose clamped start is <= row
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (max((int64_t)0, min(end, off[mid])) <= row) lo = mid; else hi = mid;
  }
  const AugScan S = scans[lo];
  const int64_t i = row - S.lo;
  if (i < 0 || i >= (int64_t)S.n) return;      // a row no scan owns (offsets that do not start at 0 or are not ascending)
  float x = pts[row * 3], y = pts[row * 3 + 1], z = pts[row * 3 + 2];
  const bool removed = aug_stage1(c, S, (uint32_t)i, x, y, z);
  const bool erased = S.block_on && S.bx0 < x && x < S.bx1 && S.by0 < y && y < S.by1;
  if (erased) x = y = z = 0.f;
  const AugSet Q = *set;
  if (c.stages & EGONN_AUG_SET_ROTATE) {
    const float nx = x * Q.c + y * Q.s, ny = x * (-Q.s) + y * Q.c;
    x = nx;
    y = ny;
  }
  if (Q.flip == 0) x = -x;
  if (Q.flip == 1) y = -y;
  if (Q.flip == 2) z = -z;
  if (c.stages & EGONN_AUG_RIGID) {
    const float nx = x * S.m[0] + y * S.m[1] + z * S.m[2] + S.m[3];
    const float ny = x * S.m[4] + y * S.m[5] + z * S.m[6] + S.m[7];
    const float nz = x * S.m[8] + y * S.m[9] + z * S.m[10] + S.m[11];
    x = nx;
    y = ny;
    z = nz;
  }
  if (S.status & EGONN_AUG_STATUS_BAD_ID) x = y = z = NAN;
  out[row * 3] = x;
  out[row * 3 + 1] = y;
  out[row * 3 + 2] = z;
  if (flags) flags[row] = (uint8_t)((removed ? 1 : 0) | (erased ? 2 : 0));
}

// the carves of the caller's scratch.  With scratch = nullptr only `total` means anything
struct AugSpan {
  AugScan* scans;
  AugSet* set;
  float* partial;
  size_t total;
};
static AugSpan aug_span(void* scratch, int B) {
  AugSpan S;
  Carve c(scratch);
  S.scans = c.take<AugScan>((size_t)B);
  S.set = c.take<AugSet>(1);
  S.partial = c.take<float>((size_t)B * AUG_CHUNKS * 6);
  S.total = c.total();
  return S;
}

}  // namespace egonn

using namespace egonn;

API int64_t egonn_augment_scratch_bytes(int64_t n, int batch_size) {
  if (n < 0 || n >= (1ll << 24) || batch_size < 1 || batch_size > EGONN_MAX_BATCH) return -1;
  return (int64_t)aug_span(nullptr, batch_size).total;
}

API int egonn_augment_points(const float* points, int64_t n, const int64_t* scan_offsets, int batch_size, const int32_t* scan_ids,
                             const egonn_augment_params* params, const float* T_in, float* out_points, float* T_out,
                             int32_t* rec_i, double* rec_d, uint8_t* flags, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(n >= 0 && n < (1ll << 24) && batch_size >= 1 && batch_size <= EGONN_MAX_BATCH, EGONN_ERR_INVALID,
                "augment: bad shape (n=%lld, batch_size=%d; n < 2^24 = the draw's point field, batch_size <= %d)", (long long)n,
                batch_size, EGONN_MAX_BATCH);
  EGONN_REQUIRE(params && scan_offsets && scratch && (n == 0 || (points && out_points)), EGONN_ERR_INVALID, "augment: null pointer");
  const egonn_augment_params c = *params;
  EGONN_REQUIRE(c.draw < (1u << 14) && c.set_id < (1u << 22), EGONN_ERR_INVALID,
                "augment: draw %u needs more than 14 bits or set_id %u more than 22", c.draw, c.set_id);
  EGONN_REQUIRE((c.stages & ~(uint32_t)EGONN_AUG_ALL) == 0, EGONN_ERR_INVALID, "augment: unknown stage bits 0x%x", c.stages);
  // a stage's parameters are checked only where its bit is set: what a switched-off stage carries is never read
  auto on = [&](uint32_t bit) { return (c.stages & bit) != 0; };
  EGONN_REQUIRE(!on(EGONN_AUG_JITTER) || (c.sigma > 0.0 && c.sigma < 1e18), EGONN_ERR_INVALID, "augment: sigma %g", c.sigma);
  EGONN_REQUIRE(!on(EGONN_AUG_JITTER_CLIP) || (c.clip >= 0.0 && c.clip < 1e18), EGONN_ERR_INVALID, "augment: clip %g", c.clip);
  EGONN_REQUIRE(!on(EGONN_AUG_REMOVE_POINTS) || (c.r_min >= 0.0 && c.r_min <= c.r_max && c.r_max <= 1.0), EGONN_ERR_INVALID,
                "augment: removal ratio range (%g, %g)", c.r_min, c.r_max);
  EGONN_REQUIRE(!on(EGONN_AUG_TRANSLATE) || (c.max_delta >= 0.0 && c.max_delta < 1e18), EGONN_ERR_INVALID,
                "augment: max_delta %g", c.max_delta);
  EGONN_REQUIRE(!on(EGONN_AUG_ROTATE) || fabs(c.max_theta) < 1e6, EGONN_ERR_INVALID, "augment: max_theta %g", c.max_theta);
  EGONN_REQUIRE(!on(EGONN_AUG_BLOCK) || (c.block_p >= 0.0 && c.block_p <= 1.0 && c.scale_lo >= 0.0 && c.scale_lo <= c.scale_hi &&
                                          c.scale_hi < 1e18 && c.ratio_lo > 0.0 && c.ratio_lo <= c.ratio_hi && c.ratio_hi < 1e18),
                EGONN_ERR_INVALID, "augment: block p %g, scale (%g, %g), ratio (%g, %g)", c.block_p, c.scale_lo, c.scale_hi,
                c.ratio_lo, c.ratio_hi);
  EGONN_REQUIRE(!on(EGONN_AUG_SET_ROTATE) || fabs(c.set_max_theta) < 1e6, EGONN_ERR_INVALID, "augment: set_max_theta %g",
                c.set_max_theta);
  EGONN_REQUIRE(!on(EGONN_AUG_FLIP) || (c.flip_cum[0] >= 0.0 && c.flip_cum[0] <= c.flip_cum[1] && c.flip_cum[1] <= c.flip_cum[2] &&
                                         c.flip_cum[2] <= 1.0),
                EGONN_ERR_INVALID, "augment: flip thresholds (%g, %g, %g)", c.flip_cum[0], c.flip_cum[1], c.flip_cum[2]);
  EGONN_REQUIRE(!on(EGONN_AUG_RIGID) || (c.rot_max >= 0.0 && c.rot_max < 1e6 && c.trans_max >= 0.0 && c.trans_max < 1e18),
                EGONN_ERR_INVALID, "augment: rot_max %g, trans_max %g", c.rot_max, c.trans_max);
  const AugSpan S = aug_span(scratch, batch_size);
  EGONN_TRY(span_check("augment", scratch, scratch_bytes, S.total));
  hipStream_t st = (hipStream_t)stream;
  AugScan* scans = S.scans;
  AugSet* set = S.set;
  float* partial = S.partial;
  hipLaunchKernelGGL(aug_select_kernel, dim3((unsigned)batch_size), dim3(AUG_SEL_WG), 0, st, scan_offsets, batch_size, n, scan_ids, c,
                     scans);
  if (c.stages & EGONN_AUG_BLOCK)
    hipLaunchKernelGGL(aug_box_kernel, dim3(AUG_CHUNKS, (unsigned)batch_size), dim3(AUG_BOX_WG), 0, st, points, scan_offsets,
                       batch_size, n, c, scans, partial);
  hipLaunchKernelGGL(aug_param_kernel, dim3((unsigned)cdiv(batch_size, 64)), dim3(64), 0, st, batch_size, c, scans, set, partial, T_in,
                     T_out, rec_i, rec_d);
  if (n > 0)
    hipLaunchKernelGGL(aug_apply_kernel, dim3((unsigned)cdiv(n, AUG_TILE)), dim3(AUG_TILE), 0, st, points, scan_offsets, batch_size, n,
                       c, scans, set, out_points, flags);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
