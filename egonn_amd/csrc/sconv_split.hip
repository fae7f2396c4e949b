// fp32 sparse convolution on the fp16 matrix pipe: two-way split operands, three products, fp32 accumulate (gfx950).
//
// Replaces the same reference operators as sconv.hip (MinkowskiConvolution k=3 / k=2,s=2 and
// MinkowskiConvolutionTranspose forward: models/minkgl.py:39,100,105 and :46-60; ME BasicBlock conv1/conv2 via
// layers/eca_block.py:58-63) for fp32 feature maps:
//
//   out[o] = act( (sum_k in[nbr[o][k]] @ W[k]) * scale + shift )
//
// Arithmetic: the project's fp16 split (split16.h: error bound, range, why weights are scaled and activations are not, the order
// of the three products, the range guard).  This file is the kernels around it.
//
// Decomposition (unchanged from round 3):
//   * a WORKGROUP of NW waves owns NW consecutive row groups (rowgroup.hip: 16 output rows each, sorted by neighbour mask
//     inside a window, so consecutive groups have nearly the same offsets present) and NSW 32-column slices;
//   * the workgroup walks the UNION of its groups' offsets k and the 32-channel blocks cb in lock-step.  Per step the slab
//     W[k][cb][its columns] (hi|lo fragments, 128*COUT bytes) is copied ONCE per workgroup global -> LDS by LDS-DMA
//     (buffer_load_dwordx4 ... lds, lane-linear = fragment order) and every wave reads its B fragments from there;
//   * every wave gathers the rows of its own group by LDS-DMA in full 128-byte lines (structured buffer: vindex = the
//     neighbour row from the table, -1 = absent = out of range = zeros without traffic; XOR-swizzled source chunk so that
//     the lane-linear LDS image is conflict-free for the ds_read_b128 fragment reads), splits them ONCE in registers
//     and feeds the MFMAs of all its column slices;
//   * DMA of step i+1 is issued at the start of step i; a wave waits for its own pieces at the end of the step and one
//     s_barrier per step publishes the slab (and retires the slab that is overwritten next);
//   * a group that lacks the offset skips the step's split and MFMAs (wave-uniform branch).
// Every output row is produced by one wave, summed in ascending k, ascending channel block, fixed term order: results do not
// depend on the batch, the grouping of other rows or eager vs graph execution (bitwise reproducible, batch-invariant).
// The compiler does not know that an LDS-DMA write feeds a later ds_read (it would drain vmcnt(0) in front of any LDS read
// it can see), so every LDS read of the step loop is issued from asm with its own counted waits.
// (The six-product bf16 kernel, its wave-wide variant and the 3 / 9-product measurement builds: tools/exp/r03_sconv_split_bf16x6.hip.)
#include <stdlib.h>
#include <algorithm>
#include <type_traits>
#include <utility>

#include "common.h"
#include <hip/hip_ext.h>
#include "kernels.h"
#include "rowmath.h"
#include "split16.h"

namespace egonn {

// ------------------------------------------------------------------ weight packing
// W[k][ci][co] -> Wsp[k][cb][ns][f][lane][e] (fp16), f = 2*part + nt, part: 0 hi, 1 lo
//   = part( s * W[k][32cb + split_chan(lane>>4, e)][32ns + 16nt + (lane&15)] ),   s = 2^(13 - exponent(max |W|))
// so that the slab of a step (k, cb) is one contiguous block of COUT/32 * 4 KB and every 1 KB piece is one lane-linear
// MFMA A-operand fragment.  Behind the fragments (split16.h: split_frag_bytes, split_pack_winv): float 1/s, uint32 bits of max |W|.
// flip / transpose: as pack_rg_weights (input-gradient kernels, k=2 <-> transposed pairs).
__global__ void split_absmax_kernel(const float* __restrict__ W, int64_t n, uint32_t* __restrict__ trailer) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const float m = split_finite_absmax(W, n, t, (int64_t)gridDim.x * blockDim.x);
  if ((threadIdx.x & 63) == 0) atomicMax(trailer + 1, __float_as_uint(m));
}
__global__ void pack_split_weights_kernel(const float* __restrict__ W, int K, int cin, int cout, int flip, int transpose,
                                          uint16_t* __restrict__ out, uint32_t* __restrict__ trailer) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t per_k = (int64_t)cin * cout;
  const float sc = split_scale_of(trailer[1]);
  if (t == 0) reinterpret_cast<float*>(trailer)[0] = 1.f / sc;
  if (t >= K * per_k * 2) return;
  const int ncb = cin / 32, ns_n = cout / 32;
  int64_t r = t;
  const int e = (int)(r & 7); r >>= 3;
  const int lane = (int)(r & 63); r >>= 6;
  const int f = (int)(r & 3); r >>= 2;
  const int ns = (int)(r % ns_n); r /= ns_n;
  const int cb = (int)(r % ncb); r /= ncb;
  const int k = (int)r;
  const int part = f >> 1, nt = f & 1;
  const int ci = 32 * cb + split_chan(lane >> 4, e);
  const int co = 32 * ns + 16 * nt + (lane & 15);
  const int ks = flip ? K - 1 - k : k;
  const float v = sc * (transpose ? W[(int64_t)ks * per_k + (int64_t)co * cin + ci] : W[(int64_t)ks * per_k + (int64_t)ci * cout + co]);
  out[t] = __builtin_bit_cast(uint16_t, split_part(v, part));
}

size_t split_weights_bytes(int K, int cin, int cout) { return split_frag_bytes(K, cin, cout) + SPLIT_TRAILER_BYTES; }
size_t sconv_split_part_floats(const RowGroups& rg, int cout, int kparts) {
  return kparts > 1 ? (size_t)kparts * rg.cap_groups * 16 * cout : 0;
}

int pack_split_weights(const float* W, int K, int cin, int cout, int flip, int transpose, void* out, hipStream_t stream) {
  EGONN_REQUIRE(cin % 32 == 0 && cout % 32 == 0, EGONN_ERR_INVALID, "sconv: channel counts must be multiples of 32 (%d->%d)", cin, cout);
  const int64_t nw = (int64_t)K * cin * cout, n = nw * 2;
  uint32_t* trailer = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(out) + split_frag_bytes(K, cin, cout));
  HIP_CHECK(hipMemsetAsync(trailer, 0, SPLIT_TRAILER_BYTES, stream));
  hipLaunchKernelGGL(split_absmax_kernel, dim3((unsigned)std::min<int64_t>(cdiv(nw, 256), 256)), dim3(256), 0, stream, W, nw, trailer);
  hipLaunchKernelGGL(pack_split_weights_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, stream, W, K, cin, cout, flip,
                     transpose, reinterpret_cast<uint16_t*>(out), trailer);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------ the kernel
struct SplitArgs {
  const float* in;           // [n_in][CIN] fp32
  const int32_t* snbr;       // row-group tables
  const uint32_t* gmask;
  const int32_t* perm;
  const int32_t* meta;       // [0] = groups in use
  const int32_t* order;      // dispatch order of the 4-group tasks (rowgroup.hip; nullable = table order)
  const void* Wsp;           // pack_split_weights
  const float* scale;        // folded BatchNorm (nullable)
  const float* shift;
  float* out;                // [n_out][COUT]
  float* psum;               // [groups][COUT] column sums of the stored values (nullable)
  uint32_t in_rows, w_bytes;
  int K, relu, cap_groups;
  int in_split, out_split;   // the input / output map is in SPLIT FORM: per row and 32-channel block the 128 bytes hold the fp16 hi
                             // parts (chunk g = channels split_chan(g, 0..7)) and lo parts (chunk 4 + g) the consumer's MFMA operands
                             // are made of, instead of 32 fp32 values.  Same size, same gather; the consumer's in-loop split
                             // (24 vector instructions per 16 x 32 fragment) moves into the producer's epilogue.  hi / lo are
                             // computed by the same split8h either way: results are bitwise those of fp32 maps.
  // GATED instantiation only: the input map does not exist — row r of it is relu(in[r] * gate[scan][c] + in2[r]) (the tail of the
  // ECA block below, layers/eca_block.py:66-73), evaluated on the gathered fragments with the expression of eca_apply_kernel
  const float* in2 = nullptr;
  const float* gate = nullptr;            // [B][CIN]
  int B = 0;
  unsigned long long* trace = nullptr;   // measurement builds only (tools/split_trace.py): 12 u64 per wave task
  // OFFSET-SPLIT launches (kp_n > 1; maps below one round of the chip): blockIdx.z = kp owns the contiguous offset range
  // [kp * K / kp_n, (kp + 1) * K / kp_n), walks only its share of the steps and leaves the RAW accumulator tiles of every group
  // that has an offset in the range in part[kp][group][slice][tile][lane] (the accumulator layout itself: 1 KB coalesced stores).
  // sconv_split_reduce_kernel sums the parts in ascending kp and applies this kernel's epilogue — the hand-over is a kernel
  // boundary, nothing is synchronised in here.
  float* part = nullptr;
  int kp_n = 1;
  // RANGE GUARD (split16.h): the plan's flag word; the epilogue sees every accumulator and raises SPLIT_RANGE_BIT on a non-finite one
  int32_t* flags = nullptr;
  // OPERAND SCALE (the input-gradient convolutions of a training step: gradients of 1e-6 .. 1e-8 would lose their low parts): the bits
  // of max |in| (split_absmax_kernel); the gathered rows are multiplied by the power of two that puts the maximum into
  // [2^13, 2^14) before they are split — what pack_split_weights does to the kernel — and the epilogue divides it out (both exact).
  const uint32_t* in_maxbits = nullptr;
  // RESIDUAL (nullable): out[row] = epilogue value + res[row] ([n_out][COUT] fp32) — the FPN step of MinkHead, `tconv(y) + conv1x1(x)`
  // (models/minkgl.py:46-60), as the transposed convolution's epilogue
  const float* res = nullptr;
};
__host__ __device__ static inline uint32_t ks_range_mask(int kp, int kp_n, int K) {      // offsets [kp*K/kp_n, (kp+1)*K/kp_n)
  const int k0 = kp * K / kp_n, k1 = (kp + 1) * K / kp_n;
  return ((1u << k1) - 1u) & ~((1u << k0) - 1u);
}

// The epilogue of one 16-row x 32-column accumulator pair (tiles nt = 0, 1 of column slice ns): undo the weight pack scale, BN
// scale/shift (+ReLU), one 16-byte store per tile (fp32 map) or the split-form chunks, optional per-group column sums.  Shared by
// the convolution kernel and by the reducer of the offset-split launches (same expression, same order: the reducer's output for
// kp_n = 1 partials would be bitwise the kernel's own).
template <int COUT>
__device__ static inline void split_epilogue(const SplitArgs& p, const f32x4& a0, const f32x4& a1, int ns, int32_t row, int gw,
                                             int l15, int g4) {
  float winv = split_pack_winv(p.Wsp, p.w_bytes);                                                       // 1 / (pack scale): a power of two
  if (p.in_maxbits) winv *= 1.f / split_scale_of(p.in_maxbits[0]);                                     // (uniform) 1 / (operand scale)
  float sums[2][4];
  f32x4 vv[2];
  if (__builtin_expect(split_nonfinite(a0, a1) != 0.f, 0) && p.flags) split_raise(p.flags);   // range guard: one test for the eight values
#pragma unroll
  for (int nt = 0; nt < 2; ++nt) {
    const int c0 = ns * 32 + nt * 16 + 4 * g4;
    f32x4 v = (nt == 0 ? a0 : a1) * winv;
    if (p.scale) {
      const f32x4 sc = *reinterpret_cast<const f32x4*>(p.scale + c0);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(p.shift + c0);
      v = v * sc + sh;
    }
    if (p.relu) {
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = fmaxf(v[u], 0.f);
    }
    if (p.res && row >= 0) v += *reinterpret_cast<const f32x4*>(p.res + (int64_t)row * COUT + c0);
    if (row >= 0 && !p.out_split) *reinterpret_cast<f32x4*>(p.out + (int64_t)row * COUT + c0) = v;
    vv[nt] = v;
#pragma unroll
    for (int u = 0; u < 4; ++u) sums[nt][u] = row >= 0 ? v[u] : 0.f;
  }
  if (p.out_split && row >= 0) {
    // this lane holds exactly the eight channels split_chan(g4, 0..7) of its row: columns 4 g4.. of tile 0 and of tile 1
    f16x8_t oh, ol;
    split8h(vv[0], vv[1], oh, ol);
    char* o = reinterpret_cast<char*>(p.out) + ((int64_t)row * COUT + ns * 32) * 4 + 16 * g4;
    *reinterpret_cast<f16x8_t*>(o) = oh;
    *reinterpret_cast<f16x8_t*>(o + 64) = ol;
  }
  if (p.psum) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int u = 0; u < 4; ++u) sums[nt][u] = row16_sum(sums[nt][u]);
    if (l15 == 0) {
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        *reinterpret_cast<f32x4*>(p.psum + (int64_t)gw * COUT + ns * 32 + nt * 16 + 4 * g4) =
            (f32x4){sums[nt][0], sums[nt][1], sums[nt][2], sums[nt][3]};
    }
  }
}

// ------------------------------------------------------------------ reducer of the offset-split launches
// One wave per (group, 32-column slice): the parts of the group's tile pair that exist (the group has an offset in the part's
// range: the same test the convolution kernel stores under) are summed in ASCENDING kp — a fixed partition and a fixed order, so
// a row's result depends on nothing but its own neighbours — and finished by split_epilogue.  Loads of up to nine parts are in
// flight at once.
template <int COUT>
__global__ __launch_bounds__(COUT * 2) void sconv_split_reduce_kernel(const SplitArgs p) {
  constexpr int NSTOT = COUT / 32;
  const int lane = threadIdx.x & 63;
  const int ns = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, g4 = lane >> 4;
  const int gw = blockIdx.x;                                   // (< cap_groups: the grid)
  // header and parts requested together: group count, mask, output rows, and up to nine parts whether they exist or not (what a
  // part without the group's offsets holds is never used: selected by the mask below) — one round trip for a launch that is
  // nothing but round trips
  const __amdgpu_buffer_rsrc_t m_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(p.meta), 0, 4, 0x00020000);
  const int ng_v = __builtin_amdgcn_raw_buffer_load_b32(m_rsrc, 0, 0, 0);
  const __amdgpu_buffer_rsrc_t g_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(p.gmask), 0, p.cap_groups * 4, 0x00020000);
  const uint32_t gm_v = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(g_rsrc, 0, gw * 4, 0);
  const int32_t row_v = p.perm[(int64_t)gw * 16 + l15];
  const float* src = p.part + ((int64_t)gw * NSTOT + ns) * 512 + lane * 4;
  const int64_t kp_stride = (int64_t)p.cap_groups * NSTOT * 512;
  f32x4 v0[9], v1[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    v0[i] = v1[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (i < p.kp_n) {                                          // uniform
      v0[i] = *reinterpret_cast<const f32x4*>(src + i * kp_stride);
      v1[i] = *reinterpret_cast<const f32x4*>(src + i * kp_stride + 256);
    }
  }
  const int ngroups = __builtin_amdgcn_readfirstlane(min(ng_v, p.cap_groups));
  const uint32_t gm = __builtin_amdgcn_readfirstlane(gm_v);
  if (gw >= ngroups || !(gm >> 31)) return;
  f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const bool has = i < p.kp_n && (gm & ks_range_mask(i, p.kp_n, p.K)) != 0;      // wave-uniform
    a0 += has ? v0[i] : zero;
    a1 += has ? v1[i] : zero;
  }
  for (int c0 = 9; c0 < p.kp_n; c0 += 9) {                     // more than nine parts: the rest in rounds of nine, existing ones only
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      const int kp = c0 + i;
      const bool has = kp < p.kp_n && (gm & ks_range_mask(kp, p.kp_n, p.K)) != 0;
      v0[i] = v1[i] = zero;
      if (has) {
        v0[i] = *reinterpret_cast<const f32x4*>(src + kp * kp_stride);
        v1[i] = *reinterpret_cast<const f32x4*>(src + kp * kp_stride + 256);
      }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) { a0 += v0[i]; a1 += v1[i]; }
  }
  split_epilogue<COUT>(p, a0, a1, ns, row_v, gw, l15, g4);
}

template <int NSW, int NW, bool GATED = false, int KW = 1>
struct SplitGeom {
  static constexpr int NS = NSW;                         // 32-column slices a workgroup owns
  static constexpr int SLAB = NS * 4096;                 // bytes of W[k][cb][its columns]: hi | lo fragments
  static constexpr int NPIECE = NS * 4;                  // 1 KB DMA pieces per slab
  static constexpr int WPP = (NPIECE + NW - 1) / NW;     // pieces a wave issues per step (at most)
  static constexpr int TBL_BYTES = 27 * 64;              // one group's table: 27 offsets x 16 slots
  static constexpr int WAVE_LDS = 2048 + 2 * 2048 + (GATED ? 2 * 2048 : 0);   // table (padded) + two ring slots of 16 x 128 B (+ two of the second operand)
  static constexpr int WAVES_AT = KW * 2 * SLAB;         // two slabs per offset part
  static constexpr int LDS_BYTES = WAVES_AT + NW * KW * WAVE_LDS;
};

// NSW: 32-column slices per workgroup (grid.y = COUT/32/NSW column parts).  Small maps (levels 3-4: a few hundred tasks, less
// than one round of the chip) are a chain of K*CIN/32 dependent steps per task; giving every column part its own workgroup
// shortens the step (fewer MFMAs, a smaller slab) and multiplies the workgroups in flight; the rows are then gathered once
// per part, which small maps can afford.  Columns are independent: the results are bitwise the same for every NSW.
// KS: the offset-split instantiation (kp_n > 1).  One task per workgroup, task = blockIdx.x (a launch of a small map is one round
// of the chip: neither the XCD slices nor the longest-first order matter), and NOTHING in front of the header loads: group
// count, masks, neighbour table and output rows are requested together — the chain in front of the first gather is two
// global round trips (header, rows) instead of five (count, order, masks, table, rows).
template <int CIN, int COUT, int NW, int NSW, bool TRACE = false, bool GATED = false, bool KS = false, int KW = 1>
__global__ __launch_bounds__(NW * KW * 64) void sconv_split_kernel(const SplitArgs p) {
  using GEO = SplitGeom<NSW, NW, GATED, KW>;
  static_assert(KW == 1 || (!GATED && !TRACE), "offset parts inside a workgroup: plain instantiations only");
  static_assert(!GATED || CIN == 32, "gated input: one channel block");
  constexpr int NS = NSW, NSTOT = COUT / 32, NCB = CIN / 32;
  static_assert(NSTOT % NSW == 0, "column parts");
  const int ns0 = blockIdx.y * NSW;                      // first column slice of this workgroup
  const float in_sc = p.in_maxbits ? split_scale_of(__builtin_amdgcn_readfirstlane((int)p.in_maxbits[0])) : 1.f;   // operand scale (a power of two)
  constexpr int SLAB = GEO::SLAB, NPIECE = GEO::NPIECE, WPP = GEO::WPP;
  static_assert(GEO::LDS_BYTES <= 160 * 1024, "LDS budget");
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  typedef __attribute__((address_space(3))) char lds_char;
  const int lane = threadIdx.x & 63;
  const int wave_id = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // KW > 1: the workgroup's waves are KW offset parts x NW groups.  Part kw walks the offsets k with k % KW == kw of its group's
  // task in lock-step with the other parts (own slab pair, own ring), so that a SIMD holds KW waves that hide each other's LDS
  // and MFMA latencies; the parts' accumulators are summed through LDS in fixed order (part 0 + part 1 + ...) after the loop.
  const int wave = KW == 1 ? wave_id : wave_id % NW;     // group of the task
  const int kw = KW == 1 ? 0 : wave_id / NW;             // offset part
  const int l15 = lane & 15, g4 = lane >> 4;
  const int K = p.K;
  char* const wl = smem + GEO::WAVES_AT + wave_id * GEO::WAVE_LDS;
  int32_t* const tbl = reinterpret_cast<int32_t*>(wl);
  char* const ring = wl + 2048;
  const uint32_t smem_addr = (uint32_t)(uintptr_t)(lds_char*)smem;
  const uint32_t wl_addr = (uint32_t)(uintptr_t)(lds_char*)wl;
  // operand read addresses inside a gathered group image: chunks g4 and 4+g4 of row l15 (XOR swizzle on the chunk index)
  const uint32_t rd0 = wl_addr + 2048 + (uint32_t)(l15 * 128 + ((g4 ^ (l15 & 7)) * 16));
  const uint32_t rd1 = wl_addr + 2048 + (uint32_t)(l15 * 128 + (((4 + g4) ^ (l15 & 7)) * 16));
  const uint32_t tb0 = wl_addr + (uint32_t)((lane >> 3) * 4);          // table entry of this lane's DMA rows (L>>3, 8+(L>>3))
  const uint32_t wrd = smem_addr + (uint32_t)(kw * 2 * SLAB + lane * 16);   // fragment read address inside a slab piece (this part's slab pair)
  const int dma_chunk = ((lane & 7) ^ (lane >> 3)) * 16;
  const int w_lane = lane * 16;

  const __amdgpu_buffer_rsrc_t a_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), (short)(CIN * 4), (int)p.in_rows, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.Wsp), 0, (int)p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t a2_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(GATED ? p.in2 : p.in), (short)(CIN * 4), (int)p.in_rows, 0x00020000);

  // (KS: the group count travels with the header's vector loads — a scalar load would be waited for in front of them)
  int ngroups = 0;
  if constexpr (!KS) ngroups = __builtin_amdgcn_readfirstlane(min(p.meta[0], p.cap_groups));
  const int ntask = (ngroups + NW - 1) / NW;
  // contiguous eighth of the tasks per XCD (block b runs on XCD b % 8): a Z-order slice of the map per L2
  const int xcd = blockIdx.x & 7, nper = gridDim.x >> 3;
  const int cpx = (ntask + 7) >> 3;

  for (int lt = KS ? 0 : (int)(blockIdx.x >> 3); lt < (KS ? 1 : cpx); lt += nper) {
    const int tslot = KS ? (int)blockIdx.x : xcd * cpx + lt;
    if (!KS && tslot >= ntask) continue;                 // workgroup-uniform
    const int task = (!KS && NW == 4 && p.order) ? __builtin_amdgcn_readfirstlane(p.order[tslot]) : tslot;   // longest tasks first
    const int g0 = task * NW;
    const int gw = g0 + wave;                            // this wave's group
    unsigned long long tr[12] = {};
    auto now = [] { return (unsigned long long)__builtin_amdgcn_s_memtime(); };
    if constexpr (TRACE) tr[0] = now();
    // ---- header: masks of the workgroup's groups, this wave's neighbour table (two 16-byte pieces per lane) and output rows,
    // requested together (indices clipped to the tables' capacity; what lies beyond the groups in use is masked out below)
    const int gwc = min(gw, p.cap_groups - 1);
    uint32_t mload = 0;
    if (lane < NW) mload = p.gmask[min(g0 + lane, p.cap_groups - 1)];
    int4 hv0 = make_int4(-1, -1, -1, -1), hv1 = make_int4(-1, -1, -1, -1);
    {
      const int n16 = K * 4;
      const int4* src = reinterpret_cast<const int4*>(p.snbr + (int64_t)gwc * K * 16);
      if (lane < n16) hv0 = src[lane];
      if (lane + 64 < n16) hv1 = src[lane + 64];
    }
    int32_t orow = p.perm[(int64_t)gwc * 16 + l15];
    if constexpr (KS) {
      const __amdgpu_buffer_rsrc_t m_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<int32_t*>(p.meta), 0, 4, 0x00020000);
      ngroups = __builtin_amdgcn_readfirstlane(min(__builtin_amdgcn_raw_buffer_load_b32(m_rsrc, 0, 0, 0), p.cap_groups));
    }
    // ---- masks: union over the workgroup (identical in every wave), own group
    if (lane >= NW || g0 + lane >= ngroups) mload = 0;
    uint32_t U = 0;
#pragma unroll
    for (int q = 0; q < NW; ++q) U |= (uint32_t)__builtin_amdgcn_readlane((int)mload, q);      // (lanes 0..NW-1 hold the masks)
    if (!(U >> 31)) continue;                            // nothing but padding groups
    uint32_t gm = (uint32_t)__builtin_amdgcn_readlane((int)mload, wave);
    const bool live = (gm >> 31) != 0;
    if constexpr (KS) {                                  // offset-split launch: this workgroup's share of the offsets (uniform)
      const uint32_t rm = ks_range_mask((int)blockIdx.z, p.kp_n, K);
      U &= rm;
      gm &= rm;
      if (!U) continue;
    }
    const uint32_t gm_all = gm;                          // (the group's offsets in this launch's range, all parts)
    int n_steps_wg = 0;                                  // KW > 1: lock-steps of the workgroup = the longest part's
    if constexpr (KW > 1) {
      constexpr uint32_t base = KW == 2 ? 0x5555555u : (KW == 3 ? 0x1249249u : 0x1111111u);     // k % KW == 0
#pragma unroll
      for (int q = 0; q < KW; ++q) n_steps_wg = max(n_steps_wg, __popc(U & (base << q) & 0x07FFFFFFu) * NCB);
      U &= base << kw;
      gm &= base << kw;
    }
    (void)gm_all;
    f32x4 gq0 = {0.f, 0.f, 0.f, 0.f}, gq1 = {0.f, 0.f, 0.f, 0.f};
    if constexpr (GATED) {
      // scan of this wave's group (a group never straddles two scans): last b with meta[1 + b] <= gw; the gate of the lane's channels
      int lo = 0, hi = p.B;
      while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (p.meta[1 + mid] <= gw) lo = mid; else hi = mid;
      }
      gq0 = *reinterpret_cast<const f32x4*>(p.gate + (int64_t)lo * CIN + 4 * g4);
      gq1 = *reinterpret_cast<const f32x4*>(p.gate + (int64_t)lo * CIN + 16 + 4 * g4);
    }

    // ---- the group's neighbour table -> wave-private LDS; output rows of the epilogue
    if (!live) orow = -1;
    if (live) {
      int4* dst = reinterpret_cast<int4*>(tbl);
      dst[lane] = hv0;
      if (lane + 64 < 27 * 4) dst[lane + 64] = hv1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");

    if constexpr (TRACE) tr[1] = now();
    // ---- step generator (scalar, identical in every wave): set bits of the union x channel blocks
    uint32_t mk = U & 0x07FFFFFFu;
    const int n_steps = KW == 1 ? __popc(mk) * NCB : n_steps_wg;
    int gen_k = 0, gen_cb = 0;
    auto gen = [&](int& k, int& cb) {                      // k = 27: past the end
      const bool need = (gen_cb == 0);
      const bool take = need && (mk != 0);
      const bool valid = !need || take;
      gen_k = take ? __builtin_ctz(mk | 0x80000000u) : gen_k;
      mk = take ? (mk & (mk - 1)) : mk;
      k = valid ? gen_k : 27;
      cb = gen_cb;
      gen_cb = (valid && gen_cb + 1 < NCB) ? gen_cb + 1 : 0;
    };
    // this wave's share of the step's requests: its pieces of the slab, the rows of its group if it has the offset.
    // Requests that would move nothing are NOT issued (a step costs a wave 0..WPP+2 vector-memory instructions): the
    // texture path is the busiest unit of these kernels (profiles/r03c_pmc_wide.txt) and an out-of-range piece costs it
    // as much as a real one.  Nothing is counted: the wave drains its queue (vmcnt(0)) before the step's barrier.
    auto issue = [&](int slot, int k, int cb, int32_t i0, int32_t i1) {
      if (k >= 27) return;
      const int woff = ((k * NCB + cb) * NSTOT + ns0) * 4096;
#pragma unroll
      for (int q = 0; q < WPP; ++q) {
        const int pc = wave + NW * q;
        if (NPIECE % NW == 0 || pc < NPIECE)
          __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (lds_char*)(smem + (kw * 2 + slot) * SLAB + pc * 1024), 16, w_lane, woff + pc * 1024, 0, 0);
      }
      if ((gm >> k) & 1u) {
        __builtin_amdgcn_struct_ptr_buffer_load_lds(a_rsrc, (lds_char*)(ring + slot * 2048), 16, i0, dma_chunk, cb * 128, 0, 0);
        __builtin_amdgcn_struct_ptr_buffer_load_lds(a_rsrc, (lds_char*)(ring + slot * 2048 + 1024), 16, i1, dma_chunk, cb * 128, 0, 0);
        if constexpr (GATED) {
          __builtin_amdgcn_struct_ptr_buffer_load_lds(a2_rsrc, (lds_char*)(ring + 4096 + slot * 2048), 16, i0, dma_chunk, cb * 128, 0, 0);
          __builtin_amdgcn_struct_ptr_buffer_load_lds(a2_rsrc, (lds_char*)(ring + 4096 + slot * 2048 + 1024), 16, i1, dma_chunk, cb * 128, 0, 0);
        }
      }
    };
    auto idx_read = [&](int k, int32_t& i0, int32_t& i1) {   // issued; awaited by the lgkmcnt(0) in front of the barrier
      if (k < 27 && ((gm >> k) & 1u)) {
        const uint32_t tb = tb0 + (uint32_t)(k * 64);
        asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %2 offset:32" : "=&v"(i0), "=&v"(i1) : "v"(tb) : "memory");
      }
    };

    f32x4 acc[NS][2];
#pragma unroll
    for (int ns = 0; ns < NS; ++ns) acc[ns][0] = acc[ns][1] = (f32x4){0.f, 0.f, 0.f, 0.f};

    auto wread = [&](uint32_t a, auto NSI, f32x4 (&w)[4]) {      // the four fragments of column slice NSI (issued): hi nt0|nt1, lo nt0|nt1
      constexpr int off = decltype(NSI)::value * 4096;
      asm volatile(
          "ds_read_b128 %0, %4 offset:%5\n\t"
          "ds_read_b128 %1, %4 offset:%5+1024\n\t"
          "ds_read_b128 %2, %4 offset:%5+2048\n\t"
          "ds_read_b128 %3, %4 offset:%5+3072"
          : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3])
          : "v"(a), "n"(off)
          : "memory");
    };
    auto wwait = [&](f32x4 (&w)[4]) {
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3])::"memory");
    };
    auto h8 = [](const f32x4& wf) { return __builtin_bit_cast(f16x8_t, wf); };
    // ---- one step of this wave's group: rows of ring slot x slab of the same slot
    auto compute = [&](int slot) {
      f32x4 ra0, ra1, rb0, rb1, w[4];
      {
        const uint32_t r0 = rd0 + (uint32_t)(slot * 2048), r1 = rd1 + (uint32_t)(slot * 2048);
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3" : "=&v"(ra0), "=&v"(ra1) : "v"(r0), "v"(r1) : "memory");
        if constexpr (GATED) {
          const uint32_t q0 = r0 + 4096u, q1 = r1 + 4096u;
          asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3" : "=&v"(rb0), "=&v"(rb1) : "v"(q0), "v"(q1) : "memory");
        }
      }
      const uint32_t wa = wrd + (uint32_t)(slot * SLAB);
      wread(wa, std::integral_constant<int, 0>{}, w);
      if constexpr (GATED) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ra0), "+v"(ra1), "+v"(rb0), "+v"(rb1)::"memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ra0), "+v"(ra1)::"memory");
      wwait(w);
      f16x8_t ah, al;
      if constexpr (GATED) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          ra0[u] = fmaxf(ra0[u] * gq0[u] + rb0[u], 0.f);        // eca_apply_kernel's expression
          ra1[u] = fmaxf(ra1[u] * gq1[u] + rb1[u], 0.f);
        }
        split8h(ra0, ra1, ah, al);
      } else if (p.in_split) { ah = __builtin_bit_cast(f16x8_t, ra0); al = __builtin_bit_cast(f16x8_t, ra1); }   // (uniform branch)
      else {
        if (in_sc != 1.f) { ra0 *= in_sc; ra1 *= in_sc; }                                                       // (uniform branch)
        split8h(ra0, ra1, ah, al);
      }
      [&]<int... NSI>(std::integer_sequence<int, NSI...>) {
        (([&] {
           f32x4 wn[4];
           if constexpr (NSI + 1 < NS) wread(wa, std::integral_constant<int, NSI + 1>{}, wn);
           __builtin_amdgcn_sched_barrier(0);
           split_mfma3(h8(w[0]), h8(w[1]), h8(w[2]), h8(w[3]), ah, al, acc[NSI][0], acc[NSI][1]);   // w[2*part + nt]
           __builtin_amdgcn_sched_barrier(0);
           if constexpr (NSI + 1 < NS) {
             wwait(wn);
#pragma unroll
             for (int i = 0; i < 4; ++i) w[i] = wn[i];
           }
         }()), ...);
      }(std::make_integer_sequence<int, NS>{});
    };

    // ---- prologue: step 0 in flight, rows of step 1 looked up
    int k0, cb0, k1, cb1;
    int32_t i0 = -1, i1 = -1;
    gen(k0, cb0);
    idx_read(k0, i0, i1);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(i0), "+v"(i1)::"memory");
    issue(0, k0, cb0, i0, i1);
    gen(k1, cb1);
    idx_read(k1, i0, i1);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(i0), "+v"(i1)::"memory");
    if constexpr (TRACE) tr[2] = now();
    __builtin_amdgcn_s_barrier();
    if constexpr (TRACE) tr[3] = now();
    // ---- main loop: requests of step i+1, arithmetic of step i, drain, barrier
    for (int i = 0; i < n_steps; ++i) {
      const int slot = i & 1;
      unsigned long long ta, tb, tc, td;
      if constexpr (TRACE) ta = now();
      issue(slot ^ 1, k1, cb1, i0, i1);
      int k2, cb2;
      gen(k2, cb2);
      idx_read(k2, i0, i1);                              // (the DMA above has read its index registers at issue)
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (TRACE) tb = now();
      const bool has = k0 < 27 && ((gm >> k0) & 1u) != 0;
      if (has) compute(slot);
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (TRACE) tc = now();
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(i0), "+v"(i1)::"memory");
      if constexpr (TRACE) td = now();
      __builtin_amdgcn_s_barrier();
      if constexpr (TRACE) {
        tr[4] += tb - ta; tr[5] += tc - tb; tr[6] += td - tc; tr[7] += now() - td; tr[8] += has ? 1 : 0;
      }
      k0 = k1; k1 = k2; cb1 = cb2;
    }
    if constexpr (TRACE) tr[9] = now();

    // ---- KW > 1: the parts' tiles through LDS (the slabs are retired: the loop ended on a barrier), summed in part order
    if constexpr (KW > 1) {
      f32x4* const red = reinterpret_cast<f32x4*>(smem);
      if (kw > 0) {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) {
          red[(((kw - 1) * NW + wave) * NS * 2 + ns * 2) * 64 + lane] = acc[ns][0];
          red[(((kw - 1) * NW + wave) * NS * 2 + ns * 2 + 1) * 64 + lane] = acc[ns][1];
        }
      }
      __syncthreads();
      if (kw == 0) {
#pragma unroll
        for (int q = 1; q < KW; ++q)
#pragma unroll
          for (int ns = 0; ns < NS; ++ns) {
            acc[ns][0] += red[(((q - 1) * NW + wave) * NS * 2 + ns * 2) * 64 + lane];
            acc[ns][1] += red[(((q - 1) * NW + wave) * NS * 2 + ns * 2 + 1) * 64 + lane];
          }
      }
    }
    // ---- epilogue: BN scale/shift (+ReLU), one 16-byte store per tile; optional per-group column sums
    if (live && kw == 0) {
      if constexpr (KS) {
        // offset-split launch: the raw tiles, in accumulator layout (sconv_split_reduce_kernel finishes them)
        if (gm_all) {
          float* dst = p.part + (((int64_t)blockIdx.z * p.cap_groups + gw) * NSTOT + ns0) * 512 + lane * 4;
#pragma unroll
          for (int ns = 0; ns < NS; ++ns) {
            *reinterpret_cast<f32x4*>(dst + ns * 512) = acc[ns][0];
            *reinterpret_cast<f32x4*>(dst + ns * 512 + 256) = acc[ns][1];
          }
        }
      } else {
#pragma unroll
        for (int ns = 0; ns < NS; ++ns) split_epilogue<COUT>(p, acc[ns][0], acc[ns][1], ns0 + ns, orow, gw, l15, g4);
      }
    }
    if constexpr (TRACE) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      tr[10] = now();
      tr[11] = (unsigned long long)n_steps;
      if (lane == 0 && p.trace) {
        unsigned long long* o = p.trace + (int64_t)gw * 12;
#pragma unroll
        for (int q = 0; q < 12; ++q) o[q] = tr[q];
      }
    }
    __builtin_amdgcn_s_barrier();                        // the next task rewrites tables and slabs
  }
}

// ------------------------------------------------------------------ the weight-resident form (CIN = COUT = 32)
// The 32->32 plans of levels 1-2 gather 2 KB of rows per (group, offset) and, in the lock-step kernel above, 4 KB of W[k] per
// workgroup and step: the same K * 4 KB (108 KB for k=3, 32 KB for the 8-slot maps) fetched again by every task.  Here a workgroup
// stages the WHOLE packed kernel into LDS once (LDS-DMA, 1 KB pieces, one wait, one barrier) and then nothing is shared any more:
//   * every wave owns one row group at a time and walks the set bits of that group's OWN mask in ascending k — no union padding,
//     no s_barrier and no vmcnt(0) in the offset loop; the waits on the wave's two-slot ring are counted (the DMA of offset j + 2
//     is requested as soon as offset j's operands are in registers, so two gathers per wave are in flight);
//   * per offset the six MFMAs run in the order of split16.h's two-tile split_mfma3 (lo*hi, hi*lo, hi*hi; column tile 0 then 1) on the same
//     accumulators: per output row the same operations in the same order — results are bitwise those of cfg 142;
//   * the next group's header (mask, table, output rows, gate) is requested while the current group computes and held in registers;
//   * groups are dealt statically: the XCD slice of the lock-step kernel (block b -> contiguous eighth b % 8 of the task slots, a
//     grid that is no multiple of 8: one slice), inside it the group slots — RowGroups::order4's longest-first tasks x 4 groups —
//     round-robin over the slice's waves.  No workgroup waits for another one; a row's result does not depend on the dealing.
template <int NW, bool GATED>
struct ResidentGeom {
  static constexpr int TBL = GATED ? 512 : 2048;         // one group's table (padded); the gated form exists for the 8-slot maps
  static constexpr int WAVE_LDS = TBL + 2 * 2048 + (GATED ? 2 * 2048 : 0);   // table + two ring slots (+ two of the second operand)
  static constexpr int lds_bytes(int K) { return K * 4096 + NW * WAVE_LDS; }
};
static_assert(ResidentGeom<8, false>::lds_bytes(27) <= 160 * 1024, "resident k=3 workgroup: LDS budget");
static_assert(ResidentGeom<8, false>::lds_bytes(8) <= 80 * 1024, "resident 8-slot workgroups: two per CU");
static_assert(ResidentGeom<12, true>::lds_bytes(8) <= 160 * 1024, "resident gated workgroup: LDS budget");

template <int NW, bool GATED>
__global__ __launch_bounds__(NW * 64) void sconv_split_resident_kernel(const SplitArgs p) {
  using GEO = ResidentGeom<NW, GATED>;
  constexpr int CIN = 32, COUT = 32, NOPS = GATED ? 4 : 2;   // NOPS: vector-memory requests of one offset
  extern __shared__ __attribute__((aligned(1024))) char smem[];
  typedef __attribute__((address_space(3))) char lds_char;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int l15 = lane & 15, g4 = lane >> 4;
  const int K = p.K;
  const float in_sc = p.in_maxbits ? split_scale_of(__builtin_amdgcn_readfirstlane((int)p.in_maxbits[0])) : 1.f;
  char* const wl = smem + K * 4096 + wave * GEO::WAVE_LDS;
  int32_t* const tbl = reinterpret_cast<int32_t*>(wl);
  char* const ring = wl + GEO::TBL;
  const uint32_t smem_addr = (uint32_t)(uintptr_t)(lds_char*)smem;
  const uint32_t wl_addr = (uint32_t)(uintptr_t)(lds_char*)wl;
  const uint32_t rd0 = wl_addr + GEO::TBL + (uint32_t)(l15 * 128 + ((g4 ^ (l15 & 7)) * 16));
  const uint32_t rd1 = wl_addr + GEO::TBL + (uint32_t)(l15 * 128 + (((4 + g4) ^ (l15 & 7)) * 16));
  const uint32_t tb0 = wl_addr + (uint32_t)((lane >> 3) * 4);
  const uint32_t wrd = smem_addr + (uint32_t)(lane * 16);
  const int dma_chunk = ((lane & 7) ^ (lane >> 3)) * 16;
  const int w_lane = lane * 16;

  const __amdgpu_buffer_rsrc_t a_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), (short)(CIN * 4), (int)p.in_rows, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.Wsp), 0, (int)p.w_bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t a2_rsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(GATED ? p.in2 : p.in), (short)(CIN * 4), (int)p.in_rows, 0x00020000);

  const int ngroups = __builtin_amdgcn_readfirstlane(min(p.meta[0], p.cap_groups));
  const int ntask = (ngroups + 3) >> 2;
  const int nx = (gridDim.x & 7) ? 1 : 8;
  const int xcd = (int)blockIdx.x % nx, lb = (int)blockIdx.x / nx, nper = (int)gridDim.x / nx;
  const int cpx = (ntask + nx - 1) / nx;
  const int nslot = 4 * cpx, stride = nper * NW;         // group slots of the slice; the slice's waves
  if (lb * NW >= nslot || xcd * cpx + ((lb * NW) >> 2) >= ntask) return;   // (workgroup-uniform) no group for any wave of it

  // ---- the packed kernel -> LDS, all pieces requested before one wait
  for (int pc = wave; pc < K * 4; pc += NW)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rsrc, (lds_char*)(smem + pc * 1024), 16, w_lane, pc * 1024, 0, 0);

  struct Hdr {
    int4 hv0, hv1;
    int32_t orow;
    uint32_t gm;
    int gw;
    f32x4 gq0, gq1;
  };
  // task of group slot s (looked up one group ahead of its use: nothing waits for it); -1: past the slice
  auto task_at = [&](int s) {
    const int tslot = xcd * cpx + (s >> 2);
    if (s >= nslot || tslot >= ntask) return -1;
    return p.order ? __builtin_amdgcn_readfirstlane(p.order[tslot]) : tslot;
  };
  int task_nx = task_at(lb * NW + wave);
  // the next group of this wave from slot s on (s: past it), header requested and nothing of it waited for; gw = -1: none left
  auto fetch = [&](int& s, Hdr& h) {
    h.gw = -1;
    h.gm = 0;
    for (; s < nslot; s += stride) {
      const int task = task_nx;
      task_nx = task_at(s + stride);
      if (task < 0) { s = nslot; break; }
      const int gw = task * 4 + (s & 3);
      if (gw >= ngroups) continue;
      h.gw = gw;
      h.gm = p.gmask[gw];                                // (bit 31 clear: a padding group, skipped when its turn comes)
      const int n16 = K * 4;
      const int4* src = reinterpret_cast<const int4*>(p.snbr + (int64_t)gw * K * 16);
      h.hv0 = h.hv1 = make_int4(-1, -1, -1, -1);
      if (lane < n16) h.hv0 = src[lane];
      if (lane + 64 < n16) h.hv1 = src[lane + 64];
      h.orow = p.perm[(int64_t)gw * 16 + l15];
      if constexpr (GATED) {
        int lo = 0, hi = p.B;                            // scan of the group: last b with meta[1 + b] <= gw
        while (hi - lo > 1) {
          const int mid = (lo + hi) >> 1;
          if (p.meta[1 + mid] <= gw) lo = mid; else hi = mid;
        }
        h.gq0 = *reinterpret_cast<const f32x4*>(p.gate + (int64_t)lo * CIN + 4 * g4);
        h.gq1 = *reinterpret_cast<const f32x4*>(p.gate + (int64_t)lo * CIN + 16 + 4 * g4);
      }
      s += stride;
      return;
    }
  };

  int s = lb * NW + wave;
  Hdr cur, nxt;
  fetch(s, cur);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();                          // the kernel is resident: the only barrier of the workgroup

  auto mfma = [](const f32x4& wf, const f16x8_t& af, f32x4& c) {
    c = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, wf), af, c, 0, 0, 0);
  };
  // the group in work: its remaining offsets, output rows, gate, the offsets in ring slots `slot` (kA) and `slot ^ 1` (kB)
  uint32_t mk = 0;
  int gw = -1, kA = 27, kB = 27, slot = 0;
  int32_t orow = -1, i0 = -1, i1 = -1;
  f32x4 gq0 = {0.f, 0.f, 0.f, 0.f}, gq1 = {0.f, 0.f, 0.f, 0.f};
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  {
    auto next_k = [&]() {                                // 27: past the end
      const int k = mk ? __builtin_ctz(mk) : 27;
      mk &= mk - 1;
      return k;
    };
    auto idx_read = [&](int k, int32_t& i0, int32_t& i1) {
      if (k < 27) {
        const uint32_t tb = tb0 + (uint32_t)(k * 64);
        asm volatile("ds_read_b32 %0, %2\n\tds_read_b32 %1, %2 offset:32" : "=&v"(i0), "=&v"(i1) : "v"(tb) : "memory");
      }
    };
    auto issue = [&](int slot, int k, int32_t i0, int32_t i1) {
      if (k >= 27) return;
      __builtin_amdgcn_struct_ptr_buffer_load_lds(a_rsrc, (lds_char*)(ring + slot * 2048), 16, i0, dma_chunk, 0, 0, 0);
      __builtin_amdgcn_struct_ptr_buffer_load_lds(a_rsrc, (lds_char*)(ring + slot * 2048 + 1024), 16, i1, dma_chunk, 0, 0, 0);
      if constexpr (GATED) {
        __builtin_amdgcn_struct_ptr_buffer_load_lds(a2_rsrc, (lds_char*)(ring + 4096 + slot * 2048), 16, i0, dma_chunk, 0, 0, 0);
        __builtin_amdgcn_struct_ptr_buffer_load_lds(a2_rsrc, (lds_char*)(ring + 4096 + slot * 2048 + 1024), 16, i1, dma_chunk, 0, 0, 0);
      }
    };
    // ---- one offset: rows of ring slot x W[k] of the resident image (the lock-step kernel's compute at NS = 1)
    auto compute = [&](int slot, int k) {
      f32x4 ra0, ra1, rb0, rb1, w[4];
      const uint32_t r0 = rd0 + (uint32_t)(slot * 2048), r1 = rd1 + (uint32_t)(slot * 2048);
      asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3" : "=&v"(ra0), "=&v"(ra1) : "v"(r0), "v"(r1) : "memory");
      if constexpr (GATED) {
        const uint32_t q0 = r0 + 4096u, q1 = r1 + 4096u;
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %3" : "=&v"(rb0), "=&v"(rb1) : "v"(q0), "v"(q1) : "memory");
      }
      const uint32_t wa = wrd + (uint32_t)(k * 4096);
      asm volatile(
          "ds_read_b128 %0, %4\n\t"
          "ds_read_b128 %1, %4 offset:1024\n\t"
          "ds_read_b128 %2, %4 offset:2048\n\t"
          "ds_read_b128 %3, %4 offset:3072"
          : "=&v"(w[0]), "=&v"(w[1]), "=&v"(w[2]), "=&v"(w[3])
          : "v"(wa)
          : "memory");
      if constexpr (GATED) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ra0), "+v"(ra1), "+v"(rb0), "+v"(rb1)::"memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(ra0), "+v"(ra1)::"memory");
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3])::"memory");
      f16x8_t ah, al;
      if constexpr (GATED) {
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          ra0[u] = fmaxf(ra0[u] * gq0[u] + rb0[u], 0.f);        // eca_apply_kernel's expression
          ra1[u] = fmaxf(ra1[u] * gq1[u] + rb1[u], 0.f);
        }
        split8h(ra0, ra1, ah, al);
      } else if (p.in_split) { ah = __builtin_bit_cast(f16x8_t, ra0); al = __builtin_bit_cast(f16x8_t, ra1); }   // (uniform branch)
      else {
        if (in_sc != 1.f) { ra0 *= in_sc; ra1 *= in_sc; }                                                       // (uniform branch)
        split8h(ra0, ra1, ah, al);
      }
      __builtin_amdgcn_sched_barrier(0);
      // written out: the order of the two-tile split_mfma3 (split16.h); w[2*part + nt]
      mfma(w[2], ah, acc0); mfma(w[3], ah, acc1);        // w lo * a hi
      mfma(w[0], al, acc0); mfma(w[1], al, acc1);        // w hi * a lo
      mfma(w[0], ah, acc0); mfma(w[1], ah, acc1);        // hi * hi
      __builtin_amdgcn_sched_barrier(0);
    };

    // ---- a group begins: padding groups skipped, its table -> wave-private LDS (the ring is drained: a group's last wait is
    // vmcnt(0), and its indices have been read), the header after it requested, its first two offsets in flight.  false: none left
    auto begin = [&]() {
      while (cur.gw >= 0 && !((uint32_t)__builtin_amdgcn_readfirstlane((int)cur.gm) >> 31)) {
        fetch(s, nxt);
        cur = nxt;
      }
      if (cur.gw < 0) return false;
      gw = cur.gw;
      orow = cur.orow;
      mk = (uint32_t)__builtin_amdgcn_readfirstlane((int)cur.gm) & 0x07FFFFFFu;
      if constexpr (GATED) { gq0 = cur.gq0; gq1 = cur.gq1; }
      {
        int4* dst = reinterpret_cast<int4*>(tbl);
        if (lane < K * 4) dst[lane] = cur.hv0;
        if (lane + 64 < K * 4) dst[lane + 64] = cur.hv1;
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      fetch(s, nxt);                                     // (older than every gather of this group)
      kA = next_k();
      kB = next_k();
      slot = 0;
      idx_read(kA, i0, i1);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(i0), "+v"(i1)::"memory");
      issue(0, kA, i0, i1);
      idx_read(kB, i0, i1);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(i0), "+v"(i1)::"memory");
      issue(1, kB, i0, i1);
      return true;
    };

    bool have = begin();
    while (have) {
      const int e_gw = gw;
      const int32_t e_orow = orow;
      acc0 = acc1 = (f32x4){0.f, 0.f, 0.f, 0.f};
      // ---- offsets: wait for offset j, compute it, request offset j + 2 into its slot.  Counted waits: what may still be in
      // flight is offset j + 1 (NOPS requests).  (The previous group's epilogue — issued behind this group's first two gathers —
      // may be younger still: the count then waits for a little more than it needs, never for less; loads and stores of one
      // wave retire in order.)
      while (kA < 27) {
        const int kC = next_k();
        idx_read(kC, i0, i1);                            // (awaited by the operand wait of compute)
        if (kB < 27) {
          if constexpr (GATED) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
          else asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        } else {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        static_assert(NOPS == (GATED ? 4 : 2), "the counted waits above");
        __builtin_amdgcn_sched_barrier(0);
        compute(slot, kA);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(i0), "+v"(i1)::"memory");
        issue(slot, kC, i0, i1);                         // (the slot's operands are in registers)
        __builtin_amdgcn_sched_barrier(0);
        kA = kB; kB = kC; slot ^= 1;
      }
      // ---- the next group's first gathers go out in front of this group's epilogue (its loads and stores run under them)
      const f32x4 e0 = acc0, e1 = acc1;
      cur = nxt;
      have = begin();
      split_epilogue<COUT>(p, e0, e1, 0, e_orow, e_gw, l15, g4);
    }
  }
}

template <int COUT>
static int launch_split_reduce(const SplitArgs& a, int64_t groups_hint, hipStream_t stream, hipEvent_t ev_stop) {
  const dim3 grid((unsigned)groups_hint);
  if (ev_stop) hipExtLaunchKernelGGL((sconv_split_reduce_kernel<COUT>), grid, dim3(COUT * 2), 0, stream, nullptr, ev_stop, 0, a);
  else hipLaunchKernelGGL((sconv_split_reduce_kernel<COUT>), grid, dim3(COUT * 2), 0, stream, a);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

template <int NW, bool GATED>
static int launch_split_resident(const SplitArgs& a, const SconvChoice& ch, hipStream_t stream) {
  using GEO = ResidentGeom<NW, GATED>;
  EGONN_REQUIRE(ch.lds == (size_t)GEO::lds_bytes(a.K) && ch.block == NW * 64 && a.K * 64 <= GEO::TBL, EGONN_ERR_STATE,
                "sconv(split, resident): the choice does not fit the instantiation (K = %d)", a.K);
  return launch_sconv<sconv_split_resident_kernel<NW, GATED>>(ch, stream, a);
}

// an offset-split layer is timed from the begin of this launch to the end of its reducer (bench.py roofline leg)
template <int CIN, int COUT, int NW, int NSW, bool TRACE = false, bool GATED = false, bool KS = false, int KW = 1>
static int launch_split(const SplitArgs& a, const SconvChoice& ch, hipStream_t stream) {
  using GEO = SplitGeom<NSW, NW, GATED, KW>;
  static_assert(GEO::LDS_BYTES <= 160 * 1024, "lock-step workgroup: LDS budget");
  EGONN_REQUIRE(ch.lds == (size_t)GEO::LDS_BYTES && ch.block == NW * KW * 64, EGONN_ERR_STATE,
                "sconv(split): the choice does not fit the instantiation");
  hipEvent_t ev_stop = nullptr;
  EGONN_TRY((launch_sconv<sconv_split_kernel<CIN, COUT, NW, NSW, TRACE, GATED, KS, KW>>(ch, stream, a, a.kp_n > 1 ? &ev_stop : nullptr)));
  return a.kp_n > 1 ? launch_split_reduce<COUT>(a, a.cap_groups, stream, ev_stop) : EGONN_OK;
}

// exactly the channel plans EGONN_SP_PLAN instantiates below (the forward plans of the trunk and heads + the two
// input-gradient plans); every other pair stays on the exact kernels of sconv.hip
bool sconv_split_supported(int cin, int cout) {
  static const int plans[][2] = {{32, 32}, {32, 64}, {64, 64}, {64, 128}, {128, 128}, {64, 32}, {128, 64}};
  for (const auto& p : plans)
    if (p[0] == cin && p[1] == cout) return true;
  return false;
}

// The instantiation table of the split kernels: it switches on the fields of the choice (sconv_choose: kernels.h) and decides nothing
int sconv_split_forward(const ConvCall& c, const SconvLaunch& l, hipStream_t stream) {
  const RowGroups& rg = *l.rg;
  const SconvChoice& ch = l.ch;
  const int cin = c.cin, cout = c.cout;
  EGONN_REQUIRE(rg.built, EGONN_ERR_STATE, "sconv: row-group tables not built");
  EGONN_REQUIRE(sconv_split_supported(cin, cout), EGONN_ERR_INVALID, "sconv(split): channel plan %d->%d not supported", cin, cout);
  EGONN_REQUIRE((uint64_t)l.n_in_cap * cin * 4 < (1ull << 32) - (1ull << 20), EGONN_ERR_INVALID,
                "sconv: input feature map of %lld rows exceeds the 4 GiB buffer-resource range", (long long)l.n_in_cap);
  if (rg.cap_groups <= 0) return EGONN_OK;
  SplitArgs a;
  a.in = reinterpret_cast<const float*>(c.in); a.snbr = rg.snbr; a.gmask = rg.gmask; a.perm = rg.perm; a.meta = rg.meta; a.Wsp = l.Wp;
  a.order = switches().no_task_order ? nullptr : rg.order4;
  a.scale = c.scale; a.shift = c.shift; a.out = reinterpret_cast<float*>(c.out); a.psum = c.psum;
  a.in_rows = (uint32_t)l.n_in_cap;
  a.w_bytes = (uint32_t)split_frag_bytes(rg.K, cin, cout);           // the fragments; the pack scale's inverse sits right behind them
  a.K = rg.K; a.relu = c.relu ? 1 : 0; a.cap_groups = rg.cap_groups;
  a.flags = l.flags;
  a.res = c.residual;
  a.in_split = (c.split_io & 1) ? 1 : 0;
  if (l.in_absmax) {                                     // operand autoscale: max |in| -> in_absmax[1] (one memset + one launch)
    EGONN_REQUIRE(!(c.split_io & 1) && !c.in2 && l.in_elems > 0, EGONN_ERR_INVALID, "sconv(split): operand scale on a plain fp32 input only");
    HIP_CHECK(hipMemsetAsync(l.in_absmax, 0, 8, stream));
    hipLaunchKernelGGL(split_absmax_kernel, dim3((unsigned)std::min<int64_t>(cdiv(l.in_elems, 1024), 1024)), dim3(256), 0, stream, a.in, l.in_elems, l.in_absmax);
    a.in_maxbits = l.in_absmax + 1;
  }
  a.out_split = (c.split_io & 2) ? 1 : 0;
  if (ch.kparts > 1) {
    EGONN_REQUIRE(l.part && l.part_floats >= sconv_split_part_floats(rg, cout, ch.kparts), EGONN_ERR_STATE,
                  "sconv(split): no scratch for the partial tiles of an offset-split launch");
    a.part = l.part;
    a.kp_n = ch.kparts;
  }
  if (ch.TRACE) a.trace = g_sconv_trace;
  if (ch.GATED) {
    EGONN_REQUIRE(c.gate && l.B >= 1, EGONN_ERR_INVALID, "sconv(split): the gated input exists for the 32->32 plan only");
    a.in2 = c.in2; a.gate = c.gate; a.B = l.B;
    if (ch.resident) return launch_split_resident<12, true>(a, ch, stream);
    return launch_split<32, 32, 4, 1, false, true>(a, ch, stream);
  }
  if (ch.resident) return launch_split_resident<8, false>(a, ch, stream);
#define EGONN_SP_KW(CI, CO, NWW, NSWW, KWW)                                                               \
  if constexpr (SplitGeom<NSWW, NWW, false, KWW>::LDS_BYTES <= 160 * 1024) {                              \
    if (ch.KW == KWW && ch.KS) return launch_split<CI, CO, NWW, NSWW, false, false, true, KWW>(a, ch, stream);  \
    if (ch.KW == KWW) return launch_split<CI, CO, NWW, NSWW, false, false, false, KWW>(a, ch, stream);    \
  }
#define EGONN_SP_LOCK1(CI, CO, NWW, NSWW)                                                                 \
  if (cin == CI && cout == CO && ch.NW == NWW && ch.NSW == NSWW && !ch.TRACE) {                           \
    if constexpr (NWW == 4 && CI >= 64) {                                                                 \
      EGONN_SP_KW(CI, CO, NWW, NSWW, 2) EGONN_SP_KW(CI, CO, NWW, NSWW, 3) EGONN_SP_KW(CI, CO, NWW, NSWW, 4) \
      if (ch.KS) return launch_split<CI, CO, NWW, NSWW, false, false, true>(a, ch, stream);               \
    }                                                                                                     \
    return launch_split<CI, CO, NWW, NSWW>(a, ch, stream);                                                \
  }
#define EGONN_SP_LOCK(CI, CO, NWW)                                                                        \
  EGONN_SP_LOCK1(CI, CO, NWW, (CO / 32))                                                                  \
  if constexpr (CO >= 64) { EGONN_SP_LOCK1(CI, CO, NWW, (CO / 64)) }                                      \
  if constexpr (CO >= 128) { EGONN_SP_LOCK1(CI, CO, NWW, (CO / 128)) }
#define EGONN_SP_LOCK_TRACE(CI, CO, NWW, NSWW)                                                            \
  if (cin == CI && cout == CO && ch.NW == NWW && ch.NSW == NSWW && ch.TRACE) return launch_split<CI, CO, NWW, NSWW, true>(a, ch, stream);
  EGONN_SP_LOCK_TRACE(32, 32, 4, 1) EGONN_SP_LOCK_TRACE(32, 32, 8, 1) EGONN_SP_LOCK_TRACE(64, 64, 4, 2)
  EGONN_SP_LOCK_TRACE(128, 128, 4, 2)                    // the small maps' shape: two column parts
#define EGONN_SP_PLAN(CI, CO) EGONN_SP_LOCK(CI, CO, 8) EGONN_SP_LOCK(CI, CO, 4)
  EGONN_SP_PLAN(32, 32)
  EGONN_SP_PLAN(32, 64)
  EGONN_SP_PLAN(64, 64)
  EGONN_SP_PLAN(64, 128)
  EGONN_SP_PLAN(128, 128)
  EGONN_SP_PLAN(64, 32)
  EGONN_SP_PLAN(128, 64)
#undef EGONN_SP_PLAN
#undef EGONN_SP_LOCK
#undef EGONN_SP_LOCK1
#undef EGONN_SP_KW
#undef EGONN_SP_LOCK_TRACE
  set_error("sconv(split): the choice for %d->%d (NW %d, NSW %d) has no instantiation", cin, cout, ch.NW, ch.NSW);
  return EGONN_ERR_INVALID;
}

}  // namespace egonn
