// Internal kernel-launcher declarations shared between the .hip translation units: only what a second translation unit calls.
// An operator that is an entry point of the C ABI and nothing else is defined beside its kernels and declared in
// include/egonn_hip.h alone (loss.hip, local_loss.hip, train.hip, netvlad_train.hip, retrieval.hip, ingest.hip, ...).
#pragma once
#include "common.h"

namespace egonn {

const char* last_error();

// sconv.hip ------------------------------------------------------------------------------------
// out[o] = act( (sum_k in[nbr[o][k]] @ W[k]) * scale + shift ) on the row-group form of a kernel map (rowgroup.hip).
bool sconv_rg_supported(int cin, int cout);
// W [K][cin][cout] (reference layout) -> item-major MFMA fragment order, fp32 or bf16; flip: W'[k] = W[K-1-k];
// transpose: the source kernel is [K][cout][cin]
int pack_rg_weights(const float* W, int K, int cin, int cout, int bf16, int flip, int transpose, void* out,
                    hipStream_t stream);
extern unsigned long long* g_sconv_trace;
// One sparse-convolution kernel in the forms the kernels read (egonn_model_finalize packs every kernel of the graph once)
struct PackedKernel {
  const void* rg32 = nullptr;    // pack_rg_weights, fp32
  const void* rg16 = nullptr;    // pack_rg_weights, bf16
  const void* split = nullptr;   // pack_split_weights: the fp16-split path of fp32 maps (null: sconv_split_supported says no)
};
// One convolution over a map of the plan.  kind 0: k=3 on `level`; 1: k=2,s=2 from level-1 into `level`; 2: transposed from
// level+1 onto `level`.  bf16: feature maps in/out and weights are bf16.
struct ConvCall {
  int kind = 0, level = 0;
  const void* in = nullptr; void* out = nullptr;
  int cin = 0, cout = 0, bf16 = 0;
  const float *scale = nullptr, *shift = nullptr;   // folded BatchNorm (nullable)
  int relu = 0;
  float* psum = nullptr;                 // (nullable) [groups][cout] per-group column sums of the output
  // the kernel: packed at finalize, or (stand-alone operators) W [K][cin][cout] in reference layout + scratch to pack it into
  const PackedKernel* packed = nullptr;
  const float* W = nullptr; float* scratch = nullptr; size_t scratch_floats = 0;
  // extras of this one call (the split kernel; the residual also in the per-tile kernel of fp32 maps, levels >= 5)
  int split_io = 0;                      // bit 0 = the input map is in split form (fp16 hi | lo per 32-channel block), bit 1 = write split form
  const float *in2 = nullptr, *gate = nullptr;   // input row r = relu(in[r] * gate[scan] + in2[r]): the tail of an ECA block, never materialised
  const float* residual = nullptr;       // out += residual ([n_out][cout] fp32) in the epilogue
};
// Kernel family a layer runs on: a function of the LAYER and the context's settings, never of the batch.  sconv_choose alone decides it.
enum SconvRoute {
  ROUTE_PLAIN,        // one thread per output (conv.hip): SCONV_PLAIN, channel plans without an MFMA instantiation
  ROUTE_SPLIT,        // lock-step fp16-split kernel (sconv_split.hip)
  ROUTE_TAIL_SPLIT,   // per-tile kernel on fp16-split arithmetic: 128->128 fp32 maps above the split level limit
  ROUTE_WG,           // workgroup-cooperative exact kernel
  ROUTE_DMA,          // LDS-DMA exact kernel (fp32 maps)
  ROUTE_RG            // per-tile exact kernel
};
// The layer of one sparse convolution, as far as the launch depends on it
struct SconvLayer {
  int kind = 0, level = 0, cin = 0, cout = 0, bf16 = 0;
  bool gated = false;      // ConvCall::in2
  int split_io = 0;        // ConvCall::split_io
  bool residual = false;   // ConvCall::residual
};
// The whole launch of one layer: the kernel instantiation that runs (template parameters a kernel does not have stay 0), its grid,
// block and dynamic LDS bytes.  sconv_choose is its only author; the instantiation tables of sconv_rg_forward /
// sconv_split_forward and launch_sconv only read it.
struct SconvChoice {
  SconvRoute route = ROUTE_RG;   // the family (profiler tags, the pack the kernel reads)
  SconvRoute kernel = ROUTE_RG;  // the kernel template: route, but ROUTE_RG for the tail split and for a traced layer on a plan
                                 // without a traced instantiation
  int NW = 0, NSW = 0, KW = 0, KS = 0, GATED = 0, TRACE = 0, resident = 0;   // split kernels (resident: sconv_split_resident_kernel<NW, GATED>)
  int KSP = 0, D = 0, G = 0, SPLIT = 0, PIPE = 0;                            // exact kernels (and NW, TRACE)
  unsigned gx = 0, gy = 1, gz = 1, block = 0;
  size_t lds = 0;
  int kparts = 1;                // split: offset parts as workgroups of grid.z (> 1: a reducer launch follows)
  int err = 0;                   // != EGONN_OK: the combination is refused (the message: last_error())
};
// The one launch tail of the sparse-convolution kernels: the dynamic-LDS attribute once per (instantiation, device), the launch
// with or without the profiler's event pair (bench.py roofline leg: time exactly this dispatch), the error check.  stop_later
// (the offset-split launcher): the stop event is not attached here but handed back for the reducer launch behind it.
template <auto Kernel, class Args>
static int launch_sconv(const SconvChoice& ch, hipStream_t stream, const Args& a, hipEvent_t* stop_later = nullptr) {
  static AttrOnce attr_done;                         // per instantiation; idempotent
  if (ch.lds > 48 * 1024 && attr_done.need()) {
    HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_done.mark();
  }
  const dim3 grid(ch.gx, ch.gy, ch.gz), block(ch.block);
  hipEvent_t* pev = prof_kernel_events();
  if (pev[0]) {
    if (stop_later) *stop_later = pev[1];
    hipExtLaunchKernelGGL(Kernel, grid, block, ch.lds, stream, pev[0], stop_later ? nullptr : pev[1], 0, a);
    pev[0] = pev[1] = nullptr;
  } else {
    hipLaunchKernelGGL(Kernel, grid, block, ch.lds, stream, a);
  }
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}
SconvChoice sconv_choose(const SconvSettings& s, const SconvLayer& l, int64_t cap_groups);
SconvSetting sconv_decode(int code);    // egonn_debug_set_naive_conv's public code
SplitCfg sconv_decode_cfg(int cfg);     // the cfg of code 1000 + cfg and of EGONN_SPLIT_CFG
SconvRoute sconv_route(const Ctx* ctx, int kind, int level, int cin, int cout, int bf16);
bool sconv_split_arithmetic(const Ctx* ctx);   // the product rule with fp16-split arithmetic allowed (no exact-fp32 / debug setting)
// name of that kernel (the profiler tags carry it: bench.py's roofline leg keys on it)
const char* sconv_kernel_name(const Ctx* ctx, int kind, int level, int cin, int cout, int bf16);
// What a launch of sconv_rg_forward / sconv_split_forward needs besides the choice
struct SconvLaunch {
  SconvChoice ch;
  const RowGroups* rg = nullptr;         // row-group form of the map
  int64_t n_in_cap = 0;                  // rows the input map can hold
  const void* Wp = nullptr;              // the kernel in the form the route reads
  int32_t* flags = nullptr;              // the plan's flag word (bit 3: fp16 range guard); split arithmetic only
  int B = 0;                             // split, gated input: scans of the batch
  float* part = nullptr; size_t part_floats = 0;           // split: scratch for the partial tiles of an offset-split launch
  uint32_t* in_absmax = nullptr; int64_t in_elems = 0;     // split, operand autoscale: 8 bytes of scratch, the elements of `in`
};
int sconv_rg_forward(const ConvCall& c, const SconvLaunch& l, hipStream_t stream);
int sconv_map(Ctx* ctx, const ConvCall& c, hipStream_t stream);
// sconv_split.hip: fp32 maps on the fp16 matrix pipe (two-way split operands, three products, fp32 accumulate)
bool sconv_split_supported(int cin, int cout);
int pack_split_weights(const float* W, int K, int cin, int cout, int flip, int transpose, void* out, hipStream_t stream);
size_t split_weights_bytes(int K, int cin, int cout);   // fragments + 16 bytes (inverse of the pack scale)
int sconv_split_forward(const ConvCall& c, const SconvLaunch& l, hipStream_t stream);
size_t sconv_split_part_floats(const RowGroups& rg, int cout, int kparts);
// Offset-split rule of the fp32 lock-step kernels: parts of the map's K offsets (1 = unsplit) and column parts per task for
// (map kind, output level) — a function of the LAYER only (the partition changes the summation order of a row)
struct KsChoice { int kparts, col_parts, kw; };
KsChoice sconv_ksplit_rule(const KsRule& rule, int kind, int level);
void sconv_ksplit_defaults(KsRule* r);                  // the product rule (+ the EGONN_KSPLIT* measurement overrides)
size_t sconv_ksplit_scratch_floats(const Ctx* ctx);    // partial-tile scratch that covers every map of the context's plan
static constexpr size_t SCONV_SCRATCH_FLOATS = (size_t)2 << 20;   // 8 MB: one packed kernel (27 x 256 x 256 fp32 = 7 MB)
// conv.hip -------------------------------------------------------------------------------------
int sconv_naive(const float* in, const int32_t* nbr, const float* W, const float* scale, const float* shift, int relu,
                float* out, int64_t n_out, int K, int cin, int cout, hipStream_t stream);
int conv0_lut_init(Ctx* ctx);      // first-layer lookup table (built once per context)
int conv0_k5_forward(Ctx* ctx, const float* feat, const float* W, int cout, const float* scale,
                     const float* shift, int relu, void* out, int out_bf16, hipStream_t stream, const void* wpk = nullptr);
int conv0_pack_unit(const float* W, void* wpk, hipStream_t stream);   // 24 KB: the unit-feature kernel's W fragments

// dense.hip ------------------------------------------------------------------------------------
enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_TANH = 2, ACT_SOFTPLUS = 3, ACT_SIGMOID = 4 };
// One 1x1 convolution / Linear layer: out[r][:] = act( (in[r] @ Wmat + bias) * scale + shift ) (+ residual[r]).  Weights and
// arithmetic are fp32; each of the three row operands may be a bf16 feature map.  Fields in the order of a designated initialiser.
struct DenseCall {
  // rows
  const void* in = nullptr; int in_bf16 = 0;
  int64_t n = 0;                         // rows the buffers hold (the capacity): sizes the grid
  const int32_t* n_dev = nullptr;        // (nullable) device-resident live row count <= n: rows from it on are not written
  // kernel
  int cin = 0, cout = 0;
  const float* W = nullptr;
  int w_out_in = 0;                      // 0: Wmat = W[cin][cout] (ME 1x1 kernel layout); 1: Wmat = W[cout][cin]^T (nn.Linear layout)
  const float* wfrag = nullptr;          // (nullable) the kernel in fragment order (dense_pack_frags): the streaming form reads it
                                         // instead of gathering W per workgroup
  // epilogue
  const float* bias = nullptr;
  const float *scale = nullptr, *shift = nullptr;   // folded BatchNorm (nullable, together)
  int act = 0;                           // Act
  const void* residual = nullptr; int res_bf16 = 0;
  const float* gate = nullptr;           // (nullable) [B][cout]: the tail of an ECA block fused into the launch,
  const int32_t* boff = nullptr;         // out = relu(residual[r] * gate[scan of r] + layer output); boff = the B + 1 row offsets
  int B = 0;                             // of the scans.  Needs dense_gate_fusable(n, cin, cout)
  // output
  void* out = nullptr; int out_bf16 = 0;
  // measurement: -1 = the product rule, 0 = never the streaming form, 1 = the streaming form (an error for other shapes);
  // the forms are bitwise the same
  int form = -1;
};
// Kernel a layer runs on: a function of (rows, cin, cout, form) and EGONN_NO_DENSE_STREAM.  dense_route alone decides it (the
// rule and its thresholds: dense.hip).
enum DenseRoute {
  DENSE_INVALID = -1,  // form 1 on a shape without a streaming form
  DENSE_NONE = 0,      // no rows: nothing to launch
  DENSE_STREAM,        // dense_stream_kernel: one 16-row tile per wave, weights from the packed fragments
  DENSE_LDS,           // dense_lds_kernel: weights resident in LDS, persistent workgroups, column blocks over grid.y
  DENSE_SMALL,         // dense_small_kernel: one memory round trip per wave
  DENSE_TILE,          // dense_kernel: 64 x 64 tiles
  DENSE_PLAIN          // dense_any_kernel: thread per output; bias + activation only, fp32 rows
};
struct DenseLaunch {   // what the route implies
  DenseRoute route = DENSE_NONE;
  unsigned gx = 0, gy = 0;
  size_t lds = 0;      // dynamic LDS bytes
  int colblk = 0;      // DENSE_LDS: output columns per block of grid.y
};
DenseRoute dense_route(int64_t n, int cin, int cout, int form);
DenseLaunch dense_launch(int64_t n, int cin, int cout, int form, int gate_scans);   // gate_scans: DenseCall::B of a gated call, else 0
int dense_forward(const DenseCall& c, hipStream_t stream);
// true: a DenseCall with a gate can run on this shape (form 0 takes the persistent LDS kernel with a single column block)
bool dense_gate_fusable(int64_t n, int cin, int cout);
// three independent (n_i, 128) @ (128, 128) products in one launch of the small kernel: fp32 rows, no epilogue.  Every n_i must
// pass dense_group3_rows (the small kernel is what dense_route gives the product alone, or there are no rows)
bool dense_group3_rows(int64_t n);
// wfrag (nullable; all three or none): the kernels in fragment order, read as 16-byte loads instead of W
int dense_small_group3(const float* const* in, const int64_t* n, const int32_t* const* n_dev, const float* const* W,
                       const float* const* wfrag, float* const* out, hipStream_t stream);
int dense_pack_frags(const float* W, int w_out_in, int cin, int cout, float* out, hipStream_t stream);   // cin * cout floats

// global_tail.hip ------------------------------------------------------------------------------
// The global descriptor decoder in its shipped sizes (Linear 128 -> 192 + ReLU, Linear 192 -> 256) and the partial sums of the
// global pooling in one launch: partial[b][chunk][256] of segment_partial_sums(decoder(g5), pow_mode), bitwise, without the hidden
// map and the decoder output in memory.  wf0 / wf1: the two (out, in) kernels in fragment order (dense_pack_frags); rows of g5 are
// read inside [boff[0], boff[B]) and below ncap only
constexpr int GTAIL_CIN = 128, GTAIL_MID = 192, GTAIL_OUT = 256;
int global_tail_fused(const float* g5, int64_t ncap, const int32_t* boff, int B, const float* wf0, const float* b0, const float* wf1,
                      const float* b1, int pow_mode, const float* p, float* partial, hipStream_t stream);

// rowwise.hip ----------------------------------------------------------------------------------
int bn_fold(const float* w, const float* b, const float* rm, const float* rv, float eps, int c, float* scale,
            float* shift, hipStream_t stream);
// n_dev (nullable, here and below): device-resident row count (<= n); n then only sizes the grid
int gather_rows(const float* in, const int32_t* perm, int64_t n, int c, float* out, hipStream_t stream,
                const int32_t* n_dev = nullptr);
// per-sample column sums, deterministic two-stage: partial[b][chunk][c]
static constexpr int SEG_CHUNKS = 32;
int segment_partial_sums(const float* in, const int32_t* boff, int B, int c, int pow_mode, const float* p,
                         float* partial, hipStream_t stream);
// out[r] = relu(x[r] * sigmoid(conv1d_k(mean_b))[c] + res[r])  (ECA gate + residual + ReLU)
int eca_apply(const float* x, const float* res, const float* partial, const int32_t* boff, int B, int64_t n, int c,
              const float* wconv, int ksize, float* out, hipStream_t stream);
// ECA gate from the per-group column sums a convolution epilogue left behind (sconv.hip): gate[b][c]
int eca_gate_groups(const float* psum, const RowGroups& rg, const int32_t* boff, int B, int c, const float* wconv, int ksize,
                    float* gate, hipStream_t stream);
// out = relu(x * gate[sample] + res); bf16: x, res and out are bf16 feature maps
int eca_apply_gate(const void* x, const void* res, const float* gate, const int32_t* boff, int B, int64_t n, int c,
                   void* out, int bf16, hipStream_t stream);
int convert_bf16_to_f32(const void* in, int64_t n, float* out, hipStream_t stream);
// GeM: out[b][c] = (mean_b clamp(x,eps)^p)^(1/p) from the pow-mode partial sums
int gem_finish(const float* partial, const int32_t* boff, int B, int c, const float* p, float* out,
               hipStream_t stream);
// SPoC (mode 0: per-sample mean of the sum-mode partials) / MAC (mode 2: per-sample max of the max-mode partials)
int pool_finish(const float* partial, const int32_t* boff, int B, int c, int mode, float* out, hipStream_t stream);
int l2_normalize_rows(float* x, int64_t n, int c, hipStream_t stream, const int32_t* n_dev = nullptr);
int add_act(const float* a, const float* b, int64_t n, int relu, float* out, hipStream_t stream);

// heads.hip ------------------------------------------------------------------------------------
// waves (16-row tiles) per workgroup of the local-heads kernels; the tests read it from here (tests/helpers.py: kernel_constant) to
// build their edge batches
constexpr int LH_WAVES = 8;
// keypoint positions (reference datasets/quantization.py:60-72, 93-103)
int keypoint_positions(const uint64_t* keys, int64_t n, int level, int cb, const float* offsets, int mode,
                       const float* step, int ignore_offsets, float* out, hipStream_t stream, const int32_t* n_dev = nullptr);
// descriptor decoder + L2 norm, keypoint regressor + keypoint_position, sigma regressor (models/minkgl.py:175-225,287-308)
// in one launch on the (n,64) local feature map; w: dw0,db0,dw1,db1, kw0,kb0,kw1,kb1, sw0,sb0,sw1,sb1 (nn.Linear layouts)
int local_heads_forward(const float* x, int64_t n, const int32_t* n_dev, const float* const* w, const uint64_t* keys,
                        int level, int cb, int mode, const float* step, int ignore_offsets, float* out_desc, float* out_kp,
                        float* out_sigma, hipStream_t stream, const float* lateral_w = nullptr, const float* lateral_res = nullptr,
                        int in_bf16 = 0, const void* split_pack = nullptr, int32_t* flags = nullptr);
// the heads' six Linear kernels as fp16 hi | lo fragments (local_heads_split_kernel): w6_dev = DEVICE array of the six weight
// pointers (dw0, dw1, kw0, kw1, sw0, sw1)
size_t local_heads_pack_bytes();
int local_heads_pack(const float* const* w6_dev, void* out, hipStream_t stream);
// top-k smallest sigma per sample, ascending, ties by row (= Z-order) — eval/evaluate.py:352-361 — and the gather of the
// selected keypoints / descriptors, one launch (workgroup = scan); out_kp / out_desc nullable
int select_topk(const float* sigma, const int32_t* boff_dev, int B, int k, const float* kp, const float* desc, int dc,
                int32_t* sel_rows /*[B][k]*/, int32_t* sel_count /*[B]*/, float* out_kp, float* out_desc, hipStream_t stream);

// netvlad.hip ------------------------------------------------------------------------------------
// NetVLAD(-GC) pooling of MinkLoc (layers/netvlad.py:18-112) over the scans of boff (DEVICE, B+1): out (B, D).  Four launches;
// weights in reference layout, bn scale/shift folded (bn_fold); ws: netvlad_workspace_floats(B, C, D) floats.
static constexpr int NV_K = 64;             // clusters (NetVLADWrapper fixes cluster_size = 64)
static constexpr int NV_MAX_CHUNKS = 32;    // row chunks per scan of the row passes
static constexpr int NV_CHUNK_ROWS = 128;   // target rows per chunk
// chunks of a scan: a function of the scan's own row count only (the summation orders of every row pass follow it)
__host__ __device__ static inline int nv_chunks(int32_t len) {
  if (len <= 0) return 0;
  const int n = (len + NV_CHUNK_ROWS - 1) / NV_CHUNK_ROWS;
  return n < NV_MAX_CHUNKS ? n : NV_MAX_CHUNKS;
}
size_t netvlad_workspace_floats(int B, int C, int D);
// the carve-outs of that workspace: per-chunk partials (X^T A | a_sum), V (B, C, 64), squared-norm partials, projection partials
void netvlad_workspace_carve(float* ws, int B, int C, float** part, float** vraw, float** sq, float** pp);
int netvlad_forward(const float* x, const int32_t* boff, int B, int C, const float* wc, const float* w2, const float* sc1,
                    const float* sh1, const float* H, int D, const float* sc2, const float* sh2, const float* wg,
                    const float* scg, const float* shg, int gating, float* out, float* ws, hipStream_t stream);

// local_loss.hip ---------------------------------------------------------------------------------
// tile constants of egonn_local_loss that the tests read from here (tests/helpers.py: kernel_constant) to build their edge batches
constexpr int LL_CLOUD_CHUNK = 1024;     // cloud points per workgroup of the keypoint -> cloud search
constexpr int LL_STATS = 16;             // floats per row of out_pair / out_batch (= EGONN_LOCAL_LOSS_STATS)

}  // namespace egonn
