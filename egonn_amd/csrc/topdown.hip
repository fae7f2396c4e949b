// One top-down step of a feature pyramid on the fp16 matrix pipe (gfx950):
//
//   out[o] = x_coarse[parent(o)] @ W_t[key(o) & 7]  (+ x_lateral[o] @ W_l)
//
// i.e. MinkowskiConvolutionTranspose(k=2, s=2) onto level l plus the lateral 1x1 convolution of the same level and their sum
// (reference models/minkfpn.py:86-91, graph.top_down).  For MinkLoc3D that is 256 -> 256 plus 64 -> 256 per level-2 row, which the
// exact path runs on v_mfma_f32_16x16x4_f32 (sconv_rg / dense kernels) in three launches with two intermediate maps.
//
// Arithmetic: the project's split arithmetic (split16.h): every fp32 operand is hi + lo in fp16, a product is the three
// v_mfma_f32_16x16x32_f16 products lo*hi, hi*lo, hi*hi accumulated in fp32, weights are scaled by a power of two at pack time
// (pack_split_weights; undone exactly in the epilogue).  The two packs carry their own scales, so the two products keep their own
// accumulators and the epilogue forms  acc_t / s_t + acc_l / s_l  — the order `tconv + lateral` of the exact sequence.
//
// Decomposition: rows come from the row-group tables of the transposed map (rowgroup.hip: groups of 16 output rows sorted by
// their slot mask, so nearly every group has ONE slot).  A workgroup of 4 waves owns 4 consecutive groups and up to 128 columns, and
// walks the union of its groups' slots k and the 32-channel blocks in lock-step; per step the slab W[k][cb] (its columns of it: 4 KB of hi | lo
// fragments per 32 columns, already in lane order) is staged ONCE per workgroup in LDS — through registers, loaded one step ahead, two LDS
// buffers, one barrier per step — and every wave that has the slot multiplies the 16 gathered rows of its group with it.  The
// lateral product is the same loop over the Cl / 32 blocks of the K = 1 pack with the group's own output rows as the gathered rows.
// Every output row has exactly one parent and one slot: its value is one fixed-order sum that depends on nothing but its own
// operands (batch-invariant, capacity-invariant, the same eager and replayed).  Plain loads with explicit bounds checks: a row
// index beyond the map's capacity (a clipped plan) reads zeros and is never stored.
#include <algorithm>

#include "model.h"
#include "split16.h"

namespace egonn {

namespace {

struct TopdownArgs {
  const float* xc;           // [n_in][C] coarse map
  const float* xl;           // [n_out][Cl] lateral map (nullable)
  const uint4* wt;           // pack_split_weights(w_tconv, 8, C, C)
  const uint4* wl;           // pack_split_weights(w_lateral, 1, Cl, C) (null with xl)
  const int32_t* snbr;       // row-group tables of the transposed map
  const uint32_t* gmask;
  const int32_t* perm;
  const int32_t* meta;
  float* out;                // [n_out][C]
  int32_t* flags;            // the plan's fp16 range word (split16.h: split_raise)
  uint32_t n_in_cap, n_out_cap;
  int cap_groups, ncl;       // ncl = Cl / 32
};

constexpr int TD_NW = 4;     // waves (= row groups) per workgroup

// C: channels of the coarse map and of the output; NS: 32-column slices a workgroup owns (blockIdx.y = column part: columns are
// independent, so the parts only gather the rows again; 256 columns in one workgroup need 415 registers per lane).  The
// workgroup's share of a step's slab is NS * 4 KB = NS * 256 uint4, contiguous inside the (C / 32) * 4 KB slab of the pack.
template <int C, int NS>
__global__ __launch_bounds__(TD_NW * 64) void topdown_split_kernel(const TopdownArgs p) {
  constexpr int NSTOT = C / 32, NCB = C / 32;
  static_assert(NSTOT % NS == 0, "column parts");
  constexpr int SLAB16 = NS * 256;                       // uint4 per workgroup and step
  constexpr int SRC16 = NSTOT * 256;                     // uint4 per (k, cb) in the pack
  const int ns0 = blockIdx.y * NS;                       // first column slice of this workgroup
  constexpr int PER_T = SLAB16 / (TD_NW * 64);           // uint4 per thread and slab (1 / 2 / 4 / 8)
  static_assert(SLAB16 % (TD_NW * 64) == 0, "slab pieces per thread");
  extern __shared__ __attribute__((aligned(16))) char td_smem[];
  uint4* const slab = reinterpret_cast<uint4*>(td_smem);                 // [2][SLAB16]
  int32_t* const tbl = reinterpret_cast<int32_t*>(td_smem + 2 * SLAB16 * 16);   // [TD_NW][8][16]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, g4 = lane >> 4;
  const int g0 = blockIdx.x * TD_NW, gw = g0 + wave;     // (< cap_groups: the grid is cap_groups / TD_NW)
  const int ngroups = min(p.meta[0], p.cap_groups);

  // masks of the workgroup's groups (identical in every thread), their union, this wave's own
  uint32_t U = 0, gm = 0;
#pragma unroll
  for (int q = 0; q < TD_NW; ++q) {
    const uint32_t m = (g0 + q < ngroups) ? p.gmask[g0 + q] : 0u;
    U |= m;
    gm = q == wave ? m : gm;
  }
  if (!(U >> 31)) return;                                // nothing but padding groups (workgroup-uniform, before any barrier)
  const bool live = (gm >> 31) != 0;
  gm = live ? (gm & 0xFFu) : 0u;
  const uint32_t U8 = U & 0xFFu;
  int32_t orow = live ? p.perm[(int64_t)gw * 16 + l15] : -1;
  if ((uint32_t)orow >= p.n_out_cap) orow = -1;          // (-1 = padding slot; beyond the capacity: a clipped plan)
  // this wave's neighbour table -> LDS (8 slots x 16 rows = 128 entries, two per lane)
  {
    const int32_t* src = p.snbr + (int64_t)gw * 128;
    tbl[wave * 128 + lane] = live ? src[lane] : -1;
    tbl[wave * 128 + 64 + lane] = live ? src[64 + lane] : -1;
  }

  const int n_t = __popc(U8) * NCB;
  const int n_steps = n_t + (p.xl ? p.ncl : 0);
  // step s -> (source slab, the row this lane gathers from which map); uniform except the row
  auto slab_of = [&](int s, bool& lateral, int& k, int& cb) -> const uint4* {
    lateral = s >= n_t;
    if (lateral) { k = 0; cb = s - n_t; return p.wl + (int64_t)cb * SRC16 + ns0 * 256; }
    int idx = s / NCB;
    cb = s - idx * NCB;
    uint32_t m = U8;
    for (int i = 0; i < idx; ++i) m &= m - 1;
    k = __builtin_ctz(m | 0x100u);
    return p.wt + ((int64_t)k * NCB + cb) * SRC16 + ns0 * 256;
  };

  uint4 wreg[PER_T];
  f32x4 an0 = {0.f, 0.f, 0.f, 0.f}, an1 = {0.f, 0.f, 0.f, 0.f};
  bool an_has = false;
  // the requests of step s: the slab (every thread its pieces) and this lane's 8 channels of its gathered row
  auto fetch = [&](int s, bool table_ready) {
    bool lateral; int k, cb;
    const uint4* src = slab_of(s, lateral, k, cb);
#pragma unroll
    for (int q = 0; q < PER_T; ++q) wreg[q] = src[q * (TD_NW * 64) + tid];
    an0 = an1 = (f32x4){0.f, 0.f, 0.f, 0.f};
    an_has = lateral ? live : (((gm >> k) & 1u) != 0);
    if (!an_has) return;
    if (lateral) {
      if (orow >= 0) {
        const float* r = p.xl + (int64_t)orow * (p.ncl * 32) + cb * 32 + 4 * g4;
        an0 = *reinterpret_cast<const f32x4*>(r);
        an1 = *reinterpret_cast<const f32x4*>(r + 16);
      }
    } else {
      const int32_t row = table_ready ? tbl[wave * 128 + k * 16 + l15] : p.snbr[(int64_t)gw * 128 + k * 16 + l15];
      if ((uint32_t)row < p.n_in_cap) {                  // -1 = the row has another slot; beyond the capacity: a clipped plan
        const float* r = p.xc + (int64_t)row * C + cb * 32 + 4 * g4;
        an0 = *reinterpret_cast<const f32x4*>(r);
        an1 = *reinterpret_cast<const f32x4*>(r + 16);
      }
    }
  };
  auto stash = [&](int buf) {
#pragma unroll
    for (int q = 0; q < PER_T; ++q) slab[buf * SLAB16 + q * (TD_NW * 64) + tid] = wreg[q];
  };

  f32x4 acc_t[NS][2], acc_l[NS][2];
#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
    acc_t[ns][0] = acc_t[ns][1] = acc_l[ns][0] = acc_l[ns][1] = (f32x4){0.f, 0.f, 0.f, 0.f};

  if (n_steps > 0) {                                     // (uniform; a live group always has a slot)
    fetch(0, false);
    stash(0);
  }
  f32x4 a0 = an0, a1 = an1;
  bool a_has = an_has;
  __syncthreads();                                       // slab 0 and the tables are published

  for (int s = 0; s < n_steps; ++s) {
    const int buf = s & 1;
    const bool lateral = s >= n_t;
    if (s + 1 < n_steps) fetch(s + 1, true);             // in flight under the arithmetic of step s
    if (a_has) {                                         // wave-uniform
      f16x8_t ah, al;
      split8h(a0, a1, ah, al);
      const uint4* w = slab + buf * SLAB16 + lane;
      auto product = [&](f32x4 (&acc)[NS][2]) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
          // fragments f = 2 * part + nt of column slice ns: hi nt0 | hi nt1 | lo nt0 | lo nt1, 64 lanes x 16 bytes each
          const f16x8_t wh0 = __builtin_bit_cast(f16x8_t, w[(ns * 4 + 0) * 64]);
          const f16x8_t wh1 = __builtin_bit_cast(f16x8_t, w[(ns * 4 + 1) * 64]);
          const f16x8_t wl0 = __builtin_bit_cast(f16x8_t, w[(ns * 4 + 2) * 64]);
          const f16x8_t wl1 = __builtin_bit_cast(f16x8_t, w[(ns * 4 + 3) * 64]);
          split_mfma3(wh0, wh1, wl0, wl1, ah, al, acc[ns][0], acc[ns][1]);
        }
      };
      if (lateral) product(acc_l); else product(acc_t);  // (uniform: the two products keep their own accumulators)
    }
    if (s + 1 < n_steps) stash(buf ^ 1);                 // (buffer buf ^ 1 was read in step s - 1: retired by that step's barrier)
    a0 = an0; a1 = an1; a_has = an_has;
    __syncthreads();
  }

  // ---- epilogue: undo the pack scales, range guard, one 16-byte store per tile
  if (!live) return;
  const float winv_t = split_pack_winv(p.wt, 8, C, C);
  const float winv_l = p.xl ? split_pack_winv(p.wl, p.ncl, 32, C) : 0.f;        // (the K = 1 pack of ncl 32-channel blocks)
  float guard = 0.f;
#pragma unroll
  for (int ns = 0; ns < NS; ++ns)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const f32x4 t = acc_t[ns][nt], l = acc_l[ns][nt];
      guard += split_nonfinite(t, l);
      if (orow >= 0) {
        f32x4 v = t * winv_t;
        if (p.xl) v = v + l * winv_l;
        *reinterpret_cast<f32x4*>(p.out + (int64_t)orow * C + (ns0 + ns) * 32 + nt * 16 + 4 * g4) = v;
      }
    }
  if (__builtin_expect(guard != 0.f, 0) && p.flags) split_raise(p.flags);
}

template <int C, int NS>
int launch_topdown(const TopdownArgs& a, hipStream_t stream) {
  constexpr int LDS = 2 * NS * 4096 + TD_NW * 128 * 4;
  static_assert(LDS <= 160 * 1024, "LDS budget");
  static AttrOnce attr_done;
  if (attr_done.need()) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&topdown_split_kernel<C, NS>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS));
    attr_done.mark();
  }
  hipLaunchKernelGGL((topdown_split_kernel<C, NS>), dim3((unsigned)(a.cap_groups / TD_NW), (unsigned)(C / 32 / NS)), dim3(TD_NW * 64), LDS,
                     stream, a);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

}  // namespace

bool topdown_split_supported(int C, int Cl) {
  return (C == 64 || C == 128 || C == 256) && (Cl == 0 || (Cl >= 32 && Cl <= C && Cl % 32 == 0));
}

int topdown_split_forward(Ctx* ctx, int level_out, const float* x_coarse, const void* sp_tconv, const float* x_lateral,
                          const void* sp_lateral, int C, int Cl, float* out, hipStream_t stream) {
  EGONN_REQUIRE(level_out >= 0 && level_out < EGONN_NUM_LEVELS - 1, EGONN_ERR_INVALID, "topdown: output level %d out of range [0,6]", level_out);
  EGONN_REQUIRE(topdown_split_supported(C, x_lateral ? Cl : 0), EGONN_ERR_INVALID,
                "topdown: channel plan C=%d, Cl=%d not supported (C 64/128/256, Cl a multiple of 32 up to C)", C, Cl);
  EGONN_REQUIRE(x_coarse && sp_tconv && out && (!x_lateral || sp_lateral), EGONN_ERR_INVALID, "topdown: null argument");
  Plan& P = ctx->plan;
  const int kind = 2;
  EGONN_TRY(ensure_rowgroups(ctx, &kind, &level_out, 1, stream));
  const RowGroups& rg = P.lv[level_out].rgT;
  EGONN_REQUIRE(rg.built && rg.K == 8 && rg.cap_groups % TD_NW == 0, EGONN_ERR_STATE, "topdown: row-group tables of the transposed map not built");
  if (rg.cap_groups == 0 || P.cap[level_out] == 0) return EGONN_OK;
  EGONN_REQUIRE(P.cap[level_out] < (1ll << 31) && P.cap[level_out + 1] < (1ll << 31), EGONN_ERR_INVALID, "topdown: map too large");
  TopdownArgs a{};
  a.xc = x_coarse; a.xl = x_lateral;
  a.wt = reinterpret_cast<const uint4*>(sp_tconv);
  a.wl = x_lateral ? reinterpret_cast<const uint4*>(sp_lateral) : nullptr;
  a.snbr = rg.snbr; a.gmask = rg.gmask; a.perm = rg.perm; a.meta = rg.meta;
  a.out = out; a.flags = ctx->dev_fp16_flag;
  a.n_in_cap = (uint32_t)P.cap[level_out + 1]; a.n_out_cap = (uint32_t)P.cap[level_out];
  a.cap_groups = rg.cap_groups; a.ncl = x_lateral ? Cl / 32 : 0;
  if (C == 64) return launch_topdown<64, 2>(a, stream);
  if (C == 128) return launch_topdown<128, 4>(a, stream);
  return launch_topdown<256, 4>(a, stream);           // two column parts
}

}  // namespace egonn
