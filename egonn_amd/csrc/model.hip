// C ABI (include/egonn_hip.h) + the EgoNN graph executor.
//
// The graph restates model_factory('egonn') (reference models/model_factory.py:31-76) and
// MinkGL.forward in eval mode (models/minkgl.py:267-315): MinkTrunk (:136-153), ECABasicBlock
// (layers/eca_block.py:56-73), MinkHead (:46-60), DescriptorDecoder / KeypointRegressor / SigmaRegressor
// (:175-225), GeM (layers/pooling.py:82-86).  Weights are addressed by the reference's state_dict keys.
#include "model.h"

using namespace egonn;

namespace {

const int PLANES[7] = {32, 64, 64, 128, 128, 128, 128};   // models/model_factory.py:40
const int GLOBAL_CH = 128, GLOBAL_DIM = 256, LOCAL_CH = 64, LOCAL_DIM = 128;

}  // namespace

// ------------------------------------------------------------------------------------------ lifecycle
API const char* egonn_last_error(void) { return last_error(); }

API int egonn_debug_set_naive_conv(egonn_ctx* c, int on) {
  EGONN_REQUIRE(c, EGONN_ERR_INVALID, "debug_set_naive_conv: null context");
  c->sconv.set = sconv_decode(on);
  return EGONN_OK;
}

// Offset-split rule of this context's fp32 sparse convolutions (tests / A-B measurements; sconv_choose): map_class 0 = the
// k=3 maps, 1 = the 8-slot maps (k=2,s=2 and transposed); kparts = offset parts as separate workgroups + reducer launch (1 = none),
// kw = offset parts inside a workgroup (0 / 1 = none, 2..4), col_parts = column parts per task (0 = automatic).  -1 keeps a field.
API int egonn_debug_set_ksplit(egonn_ctx* c, int map_class, int level, int kparts, int kw, int col_parts) {
  EGONN_REQUIRE(c && (map_class == 0 || map_class == 1) && level >= 0 && level < EGONN_NUM_LEVELS, EGONN_ERR_INVALID,
                "debug_set_ksplit: bad argument");
  EGONN_REQUIRE(kparts <= 27 && kw <= 4 && col_parts <= 4, EGONN_ERR_INVALID, "debug_set_ksplit: kparts <= 27, kw <= 4, col_parts <= 4");
  if (kparts >= 0) c->sconv.ks_rule.kparts[map_class][level] = (int8_t)std::max(kparts, 1);
  if (kw >= 0) c->sconv.ks_rule.kw[map_class][level] = (int8_t)kw;
  if (col_parts >= 0) c->sconv.ks_rule.col_parts[level] = (int8_t)col_parts;
  return EGONN_OK;
}

// Weight-resident form of the 32->32 split convolutions (sconv_choose): layers it runs on, -1 = the product rule; workgroups
// per resident launch, 0 = default
API int egonn_debug_set_resident(egonn_ctx* c, int mask, int max_workgroups) {
  EGONN_REQUIRE(c && mask >= -1 && mask <= 7 && max_workgroups >= 0 && max_workgroups <= 65536, EGONN_ERR_INVALID,
                "debug_set_resident: mask in [-1, 7], max_workgroups in [0, 65536]");
  c->sconv.resident_mask = mask < 0 ? SCONV_RESIDENT_DEFAULT : mask;
  c->sconv.resident_wgs = max_workgroups;
  return EGONN_OK;
}

API int egonn_ctx_create(egonn_ctx** out, int device, int coord_bits) {
  EGONN_REQUIRE(out != nullptr, EGONN_ERR_INVALID, "ctx_create: null out pointer");
  EGONN_REQUIRE(coord_bits >= 10 && coord_bits <= 16, EGONN_ERR_INVALID, "coord_bits=%d outside [10,16]", coord_bits);
  int ndev = 0;
  HIP_CHECK(hipGetDeviceCount(&ndev));
  EGONN_REQUIRE(device >= 0 && device < ndev, EGONN_ERR_INVALID, "device %d not present (%d HIP devices)", device, ndev);
  HIP_CHECK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_CHECK(hipGetDeviceProperties(&prop, device));
  EGONN_REQUIRE(strncmp(prop.gcnArchName, "gfx950", 6) == 0, EGONN_ERR_INVALID,
                "libegonn_hip is built for gfx950 (MI355X) only; device %d is %s", device, prop.gcnArchName);
  egonn_ctx* c = new egonn_ctx();
  c->device = device;
  c->coord_bits = coord_bits;
  // pinned staging: counts + flags (32), per-level sample offsets, and the scan offsets of egonn_voxelize (int64)
  const size_t hc = sizeof(int32_t) * (32 + (size_t)EGONN_NUM_LEVELS * (EGONN_MAX_BATCH + 1)) + sizeof(int64_t) * (EGONN_MAX_BATCH + 2);
  if (hipHostMalloc(reinterpret_cast<void**>(&c->host_counts), hc) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&c->dev_counts), sizeof(int32_t) * 32) != hipSuccess ||
      hipMalloc(reinterpret_cast<void**>(&c->dev_pairs), sizeof(unsigned long long) * 16) != hipSuccess) {
    set_error("ctx_create: allocation failed");
    delete c;
    return EGONN_ERR_HIP;
  }
  c->dev_flags = c->dev_counts + 16;   // counts[0..11], flags at [16], the fp16 range flag at [17]: fetched by one copy
  c->dev_fp16_flag = c->dev_counts + 17;
  sconv_ksplit_defaults(&c->sconv.ks_rule);
  if (conv0_lut_init(c) != EGONN_OK) {
    egonn_ctx_destroy(c);
    return EGONN_ERR_HIP;
  }
  *out = c;
  return EGONN_OK;
}

API void egonn_ctx_destroy(egonn_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  c->plan_arena.release();
  c->work_arena.release();
  c->sort_arena.release();
  if (c->host_counts) (void)hipHostFree(c->host_counts);
  if (c->dev_counts) (void)hipFree(c->dev_counts);
  if (c->dev_pairs) (void)hipFree(c->dev_pairs);
  if (c->conv0_lut) (void)hipFree(c->conv0_lut);

  for (auto& r : c->prof.recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (auto& r : c->prof.graph_recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
  for (auto e : c->prof.pool) (void)hipEventDestroy(e);
  delete c;
}

// ------------------------------------------------------------------------------------------ plan
API int egonn_voxelize(egonn_ctx* c, const float* points, const int64_t* scan_offsets, int B, int mode,
                       const float* step, void* stream) {
  EGONN_REQUIRE(c && points && scan_offsets && step, EGONN_ERR_INVALID, "voxelize: null argument");
  HIP_CHECK(hipSetDevice(c->device));
  for (int l = 0; l < EGONN_NUM_LEVELS; ++l) c->level_feat[l] = nullptr;
  c->plan_stream = (hipStream_t)stream;
  EGONN_TRY(plan_from_points(c, points, scan_offsets, 0, 0, B, mode, step, (hipStream_t)stream));
  c->from_points = true;
  return EGONN_OK;
}

API int egonn_ctx_reserve(egonn_ctx* c, int64_t max_points, int batch_size, const int64_t* level_capacity) {
  EGONN_REQUIRE(c, EGONN_ERR_INVALID, "ctx_reserve: null context");
  HIP_CHECK(hipSetDevice(c->device));
  for (int l = 0; l < EGONN_NUM_LEVELS; ++l) c->level_feat[l] = nullptr;
  return plan_reserve(c, max_points, batch_size, level_capacity);
}

API int egonn_voxelize_device(egonn_ctx* c, const float* points, int64_t n_rows, const int64_t* scan_offsets_dev, int B,
                              int mode, const float* step, void* stream) {
  EGONN_REQUIRE(c && points && scan_offsets_dev && step, EGONN_ERR_INVALID, "voxelize_device: null argument");
  HIP_CHECK(hipSetDevice(c->device));
  for (int l = 0; l < EGONN_NUM_LEVELS; ++l) c->level_feat[l] = nullptr;
  c->plan_stream = (hipStream_t)stream;
  EGONN_TRY(plan_from_points(c, points, scan_offsets_dev, n_rows, 1, B, mode, step, (hipStream_t)stream));
  c->from_points = true;
  return EGONN_OK;
}

API int egonn_level_capacity(egonn_ctx* c, int level, int64_t* cap) {
  EGONN_REQUIRE(c && c->plan.valid, EGONN_ERR_STATE, "no coordinate plan (call egonn_voxelize / egonn_coords_set first)");
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS && cap, EGONN_ERR_INVALID, "level %d out of range", level);
  *cap = c->plan.cap[level];
  return EGONN_OK;
}

// ---- hipGraph capture of a sequence of library calls (thin wrappers, so that a host without a HIP binding can use them)
struct egonn_graph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
};
API int egonn_graph_begin(void* stream) {
  HIP_CHECK(hipStreamBeginCapture((hipStream_t)stream, hipStreamCaptureModeThreadLocal));
  return EGONN_OK;
}
API int egonn_graph_end(void* stream, egonn_graph** out) {
  EGONN_REQUIRE(out, EGONN_ERR_INVALID, "graph_end: null out pointer");
  egonn_graph* g = new egonn_graph();
  hipError_t e = hipStreamEndCapture((hipStream_t)stream, &g->graph);
  if (e == hipSuccess) e = hipGraphInstantiate(&g->exec, g->graph, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    set_error("graph_end: %s (a captured call allocated or synchronised: reserve the context and run the sequence once "
              "before capturing)", hipGetErrorString(e));
    if (g->graph) (void)hipGraphDestroy(g->graph);
    delete g;
    return EGONN_ERR_HIP;
  }
  *out = g;
  return EGONN_OK;
}
API int egonn_graph_launch(egonn_graph* g, void* stream) {
  EGONN_REQUIRE(g && g->exec, EGONN_ERR_INVALID, "graph_launch: null graph");
  HIP_CHECK(hipGraphLaunch(g->exec, (hipStream_t)stream));
  return EGONN_OK;
}
API void egonn_graph_destroy(egonn_graph* g) {
  if (!g) return;
  if (g->exec) (void)hipGraphExecDestroy(g->exec);
  if (g->graph) (void)hipGraphDestroy(g->graph);
  delete g;
}

API int egonn_plan_status(egonn_ctx* c, void* stream) {
  EGONN_REQUIRE(c && (c->plan.valid || c->plan.built_reserved), EGONN_ERR_STATE,
                "no coordinate plan (call egonn_voxelize / egonn_coords_set first)");
  HIP_CHECK(hipSetDevice(c->device));
  if (c->plan.built_reserved) c->plan.valid = true;   // a replayed graph rebuilt the plan behind the host's back
  c->plan.exact = false;                 // read the state again: sizes (reserved plans) and the flags launches raise after the
  return plan_sync(c, (hipStream_t)stream);   // plan was built (range guard of the fp16-split convolutions)
}

// fp32 feature maps: on = 1 runs every sparse convolution of this context on the exact fp32 kernels (v_mfma_f32_16x16x4_f32, the
// full fp32 range), on = 0 (default) the levels <= 5 on the fp16-split matrix pipe (sconv_split.hip: |activation| < 65504, guarded:
// egonn_plan_status reports EGONN_STATUS_FP16_RANGE).  The choice is per context and a function of the layer, never of the batch.
// on = 1: every fp32 sparse convolution of this context on the fp16-split pipe first takes max |input| (one reduction launch) and scales
// the gathered rows by the power of two that puts it into [2^13, 2^14), undone exactly in the epilogue — what the kernels do to their
// weights.  For operands far below 1 (the input-gradient convolutions of a training step, egonn_amd/train.py): an fp16 low part
// flushes below 2^-25 and carries 2^-25 absolute error below 2^-14.  Eager plans only (the element count comes from the host).
API int egonn_ctx_set_operand_autoscale(egonn_ctx* c, int on) {
  EGONN_REQUIRE(c && (on == 0 || on == 1), EGONN_ERR_INVALID, "ctx_set_operand_autoscale: bad argument");
  EGONN_REQUIRE(!on || !c->reserved, EGONN_ERR_STATE,
                "ctx_set_operand_autoscale: eager plans only — the scale reads the map's row count on the host, which a reserved "
                "(egonn_ctx_reserve) plan keeps on the device");
  c->sconv.operand_autoscale = on;
  return EGONN_OK;
}

// on = 1: egonn_forward materialises the block output of EVERY level (egonn_forward_level_features(ctx, 1, ...) then has a map to
// return): level 1's block tail runs as its own launch instead of inside level 2's strided convolution (bitwise the same result).
API int egonn_debug_keep_level_features(egonn_ctx* c, int on) {
  EGONN_REQUIRE(c && (on == 0 || on == 1), EGONN_ERR_INVALID, "debug_keep_level_features: bad argument");
  c->keep_level_features = on;
  return EGONN_OK;
}

API int egonn_ctx_set_exact_fp32(egonn_ctx* c, int on) {
  EGONN_REQUIRE(c && (on == 0 || on == 1), EGONN_ERR_INVALID, "ctx_set_exact_fp32: bad argument");
  c->sconv.split_max_level = on ? -1 : 5;
  return EGONN_OK;
}

API int egonn_coords_set(egonn_ctx* c, const int32_t* coords, int64_t n, int B, void* stream) {
  EGONN_REQUIRE(c && coords, EGONN_ERR_INVALID, "coords_set: null argument");
  HIP_CHECK(hipSetDevice(c->device));
  for (int l = 0; l < EGONN_NUM_LEVELS; ++l) c->level_feat[l] = nullptr;
  c->plan_stream = (hipStream_t)stream;
  EGONN_TRY(plan_from_coords(c, coords, n, B, (hipStream_t)stream));
  c->from_points = false;
  return EGONN_OK;
}

API int egonn_level_count(egonn_ctx* c, int level, int64_t* n) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(level >= 0 && level < EGONN_MAX_LEVELS && n, EGONN_ERR_INVALID, "level %d out of range", level);
  EGONN_TRY(plan_sync(c, c->plan_stream));
  *n = c->plan.lv[level].n;
  return EGONN_OK;
}

API int egonn_level_batch_offsets(egonn_ctx* c, int level, int64_t* off) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS && off, EGONN_ERR_INVALID, "level %d out of range", level);
  EGONN_TRY(plan_sync(c, c->plan_stream));
  for (int b = 0; b <= c->plan.batch; ++b) off[b] = c->plan.boff_host[level][b];
  return EGONN_OK;
}

API int egonn_level_coords(egonn_ctx* c, int level, int32_t* out, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  return plan_level_coords(c, level, out, (hipStream_t)stream);
}

__global__ void input_index_kernel(const int32_t* __restrict__ perm0, const uint64_t* __restrict__ keys, int64_t n,
                                   int bshift, const int64_t* __restrict__ scan_off, int64_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int64_t v = perm0[i];
  if (scan_off) v -= scan_off[(int)(keys[i] >> bshift)];
  out[i] = v;
}

API int egonn_input_index(egonn_ctx* c, int64_t* out, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  EGONN_TRY(plan_sync(c, c->plan_stream));
  const Level& L = c->plan.lv[0];
  if (L.n == 0) return EGONN_OK;
  hipLaunchKernelGGL(input_index_kernel, dim3((unsigned)cdiv(L.n, 256)), dim3(256), 0, (hipStream_t)stream,
                     c->plan.perm0, L.keys, L.n, 3 * c->plan.coord_bits, c->from_points ? c->plan.scan_off : nullptr,
                     out);
  HIP_CHECK(hipGetLastError());
  return EGONN_OK;
}

// ------------------------------------------------------------------------------------------ operators
// a convolution of a stand-alone operator entry point: the kernel in reference layout, packed into the work arena per call
static int op_conv(egonn_ctx* c, int kind, int level, const void* in, int cin, const float* kernel, int cout, int bf16,
                   const float* scale, const float* shift, int relu, void* out, float* psum, void* stream) {
  Arena* A;
  EGONN_TRY(claim_work(c, (SCONV_SCRATCH_FLOATS + sconv_ksplit_scratch_floats(c)) * sizeof(float) + 8192, true, &A));
  WALLOC(float, scratch, SCONV_SCRATCH_FLOATS);
  const ConvCall cc{.kind = kind, .level = level, .in = in, .out = out, .cin = cin, .cout = cout, .bf16 = bf16, .scale = scale,
                    .shift = shift, .relu = relu, .psum = psum, .W = kernel, .scratch = scratch, .scratch_floats = SCONV_SCRATCH_FLOATS};
  return sconv_map(c, cc, (hipStream_t)stream);
}

API int egonn_conv(egonn_ctx* c, int level_in, int level_out, int ks, const float* in, int cin, const float* kernel,
                   int cout, const float* scale, const float* shift, int relu, float* out, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  EGONN_REQUIRE(level_in >= 0 && level_in < EGONN_NUM_LEVELS && level_out >= level_in && level_out < EGONN_NUM_LEVELS,
                EGONN_ERR_INVALID, "conv: levels (%d,%d) out of range", level_in, level_out);
  const Plan& P = c->plan;
  if (ks == 1) {
    EGONN_REQUIRE(level_in == level_out, EGONN_ERR_INVALID, "1x1 conv cannot change the level");
    return dense_forward({.in = in, .n = P.lv[level_in].n, .cin = cin, .cout = cout, .W = kernel, .scale = scale, .shift = shift,
                          .act = relu ? ACT_RELU : ACT_NONE, .out = out},
                         st);
  }
  if (ks == 5) {
    EGONN_REQUIRE(level_in == 0 && level_out == 0 && cin == 1, EGONN_ERR_INVALID,
                  "k=5 convolution is implemented for the stride-1 input layer with Cin=1 only");
    return conv0_k5_forward(c, in, kernel, cout, scale, shift, relu, out, 0, st);
  }
  if (ks == 3) {
    EGONN_REQUIRE(level_in == level_out && level_in >= 1, EGONN_ERR_INVALID,
                  "k=3 convolution is implemented for levels 1..7 (same in/out level)");
    return op_conv(c, 0, level_out, in, cin, kernel, cout, 0, scale, shift, relu, out, nullptr, st);
  }
  if (ks == 2) {
    EGONN_REQUIRE(level_out == level_in + 1, EGONN_ERR_INVALID, "k=2,s=2 convolution maps level l to l+1");
    return op_conv(c, 1, level_out, in, cin, kernel, cout, 0, scale, shift, relu, out, nullptr, st);
  }
  set_error("conv: kernel_size %d not supported (1, 2, 3, 5)", ks);
  return EGONN_ERR_INVALID;
}

API int egonn_conv_transpose(egonn_ctx* c, int level_in, const float* in, int cin, const float* kernel, int cout,
                             float* out, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  EGONN_REQUIRE(level_in >= 1 && level_in < EGONN_NUM_LEVELS, EGONN_ERR_INVALID,
                "transposed conv: input level %d out of range [1,7]", level_in);
  if (level_in == 1) EGONN_TRY(ensure_level0_parent_table(c, (hipStream_t)stream));
  return op_conv(c, 2, level_in - 1, in, cin, kernel, cout, 0, nullptr, nullptr, 0, out, nullptr, stream);
}

// Sparse convolution on a map of the plan with explicit precision (the operator behind egonn_conv / egonn_conv_transpose).
API int egonn_sparse_conv(egonn_ctx* c, int map_kind, int level_out, const void* in, int cin, const float* kernel, int cout,
                          int bf16, const float* scale, const float* shift, int relu, void* out, float* group_sums,
                          void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  EGONN_REQUIRE(in && kernel && out, EGONN_ERR_INVALID, "sparse_conv: null argument");
  return op_conv(c, map_kind, level_out, in, cin, kernel, cout, bf16, scale, shift, relu, out, group_sums, stream);
}
// Row-group tables of every kernel map of the plan a training step (or a sequence of stand-alone operator calls) uses, in ONE
// launch: k=3 and k=2,s=2 maps of levels 1..7, transposed maps onto levels 0..6 (with_level0_transpose: the input gradient of the
// first strided convolution; builds the level-0 parent table).  Without it every operator builds its map's tables on first
// use — 21 launches of 12 us per training step.
API int egonn_prepare_maps(egonn_ctx* c, int with_level0_transpose, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  const int tlevels[EGONN_NUM_LEVELS - 1] = {0, 1, 2, 3, 4, 5, 6}, skip = with_level0_transpose ? 0 : 1;
  return ensure_graph_rowgroups(c, EGONN_NUM_LEVELS - 1, tlevels + skip, EGONN_NUM_LEVELS - 1 - skip, (hipStream_t)stream);
}

// Measurement hook (tools/sconv_trace.py): device buffer the traced conv build (debug variant 128) writes its per-task
// timestamps into (8 u64 per wave task); null switches it off.
API int egonn_debug_set_trace(void* buf) {
  g_sconv_trace = reinterpret_cast<unsigned long long*>(buf);
  return EGONN_OK;
}

// Measurement hook (tools/rowgroup_stats.py): device copies of a map's row-group tables.  gmask_out: [groups] u32;
// snbr_out: [groups][K][16] i32 (nullable).  Returns the number of groups copied (<= capacity_groups).  [SYNC]
API int egonn_debug_rowgroup_tables(egonn_ctx* c, int map_kind, int level_out, uint32_t* gmask_out, int32_t* snbr_out,
                                    int64_t capacity_groups, int64_t* n_groups, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  EGONN_REQUIRE(n_groups && gmask_out, EGONN_ERR_INVALID, "rowgroup_tables: null argument");
  EGONN_TRY(ensure_rowgroups(c, &map_kind, &level_out, 1, (hipStream_t)stream));
  const Level& V = c->plan.lv[level_out];
  const RowGroups& rg = map_kind == 0 ? V.rg27 : (map_kind == 1 ? V.rg8 : V.rgT);
  int32_t ng = 0;
  HIP_CHECK(hipMemcpyAsync(&ng, rg.meta, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  EGONN_REQUIRE(ng <= capacity_groups, EGONN_ERR_INVALID, "rowgroup_tables: %d groups, room for %lld", ng, (long long)capacity_groups);
  HIP_CHECK(hipMemcpyAsync(gmask_out, rg.gmask, (size_t)ng * sizeof(uint32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (snbr_out)
    HIP_CHECK(hipMemcpyAsync(snbr_out, rg.snbr, (size_t)ng * rg.K * 16 * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  *n_groups = ng;
  return EGONN_OK;
}

// Test hook (tests/test_gpu_maps.py): device copy of a map's perm table, [groups][16] i32, the output row of every slot (-1 =
// padding) — with gmask and snbr of the hook above the whole row-group form.  [SYNC]
API int egonn_debug_rowgroup_perm(egonn_ctx* c, int map_kind, int level_out, int32_t* perm_out, int64_t capacity_groups,
                                  int64_t* n_groups, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  EGONN_REQUIRE(n_groups && perm_out, EGONN_ERR_INVALID, "rowgroup_perm: null argument");
  EGONN_TRY(ensure_rowgroups(c, &map_kind, &level_out, 1, (hipStream_t)stream));
  const Level& V = c->plan.lv[level_out];
  const RowGroups& rg = map_kind == 0 ? V.rg27 : (map_kind == 1 ? V.rg8 : V.rgT);
  int32_t ng = 0;
  HIP_CHECK(hipMemcpyAsync(&ng, rg.meta, sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  EGONN_REQUIRE(ng <= capacity_groups, EGONN_ERR_INVALID, "rowgroup_perm: %d groups, room for %lld", ng, (long long)capacity_groups);
  HIP_CHECK(hipMemcpyAsync(perm_out, rg.perm, (size_t)ng * 16 * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  *n_groups = ng;
  return EGONN_OK;
}

// Number of row groups (16 output rows each) of a map: rows of the `group_sums` output of egonn_sparse_conv; the groups of
// sample b are [first_group[b], first_group[b+1]) (HOST copy, B+1 entries).  [SYNC]
API int egonn_map_groups(egonn_ctx* c, int map_kind, int level_out, int64_t* n_groups, int64_t* first_group, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  EGONN_REQUIRE(n_groups, EGONN_ERR_INVALID, "map_groups: null argument");
  EGONN_TRY(ensure_rowgroups(c, &map_kind, &level_out, 1, (hipStream_t)stream));
  const Level& V = c->plan.lv[level_out];
  const RowGroups& rg = map_kind == 0 ? V.rg27 : (map_kind == 1 ? V.rg8 : V.rgT);
  std::vector<int32_t> h((size_t)c->plan.batch + 2);
  HIP_CHECK(hipMemcpyAsync(h.data(), rg.meta, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  *n_groups = h[0];
  if (first_group)
    for (int b = 0; b <= c->plan.batch; ++b) first_group[b] = h[1 + b];
  return EGONN_OK;
}

// the pooling operators: `method` over the rows of level `level`, out (B, channels)
static int op_pool(egonn_ctx* c, Pooling method, int level, const float* x, int channels, const float* p, float* out, void* stream) {
  const int B = c->plan.batch;
  Arena* A;
  EGONN_TRY(claim_work(c, (size_t)B * SEG_CHUNKS * channels * 4 + 4096, false, &A));
  WALLOC(float, partial, (size_t)B * SEG_CHUNKS * channels);
  return global_pool(method, x, c->plan.lv[level].boff, B, channels, p, partial, out, (hipStream_t)stream);
}

// SPoC pooling over the rows of level `level` (MinkowskiGlobalAvgPooling, layers/pooling.py:59-69): out (B, ch)
API int egonn_global_avg_pool(egonn_ctx* c, int level, const float* in, int ch, float* out, void* stream) {
  REQUIRE_PLAN(c);
  HIP_CHECK(hipSetDevice(c->device));
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS, EGONN_ERR_INVALID, "level %d out of range", level);
  return op_pool(c, POOL_SPOC, level, in, ch, nullptr, out, stream);
}

// eval-mode MinkowskiBatchNorm folded to scale/shift (nn.BatchNorm1d eps as given): scale = w / sqrt(var + eps)
API int egonn_bn_fold(const float* weight, const float* bias, const float* running_mean, const float* running_var,
                      float eps, int channels, float* scale, float* shift, void* stream) {
  EGONN_REQUIRE(weight && bias && running_mean && running_var && scale && shift && channels > 0, EGONN_ERR_INVALID,
                "bn_fold: bad argument");
  return bn_fold(weight, bias, running_mean, running_var, eps, channels, scale, shift, (hipStream_t)stream);
}

// Tail of a residual block on level `level`:  out = relu(x * gate + residual)
//   eca_weight != NULL: gate = sigmoid(conv1d_k(per-sample mean of x))  (ECABasicBlock, layers/eca_block.py:21-36,66-71)
//   eca_weight == NULL: gate = 1                                        (ME BasicBlock: out += residual; relu)
API int egonn_block_tail(egonn_ctx* c, int level, const float* x, const float* residual, int channels,
                         const float* eca_weight, int eca_ksize, float* out, void* stream) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS && x && residual && out, EGONN_ERR_INVALID, "block_tail: bad argument");
  HIP_CHECK(hipSetDevice(c->device));
  const int B = c->plan.batch;
  const Level& L = c->plan.lv[level];
  Arena* A;
  EGONN_TRY(claim_work(c, ((size_t)B * SEG_CHUNKS * channels + (size_t)B * channels + 64) * 4 + 4096, false, &A));
  WALLOC(float, partial, (size_t)B * SEG_CHUNKS * channels + (size_t)B * channels);
  return block_tail(x, residual, L.boff, B, L.n, channels, eca_weight, eca_ksize, partial, out, (hipStream_t)stream);
}

// SparseTensor + SparseTensor on the same coordinate map (models/minkfpn.py:91, minkgl.py:56): out = a + b
API int egonn_add(const float* a, const float* b, int64_t n, float* out, void* stream) {
  EGONN_REQUIRE(a && b && out && n >= 0, EGONN_ERR_INVALID, "add: bad argument");
  return add_act(a, b, n, 0, out, (hipStream_t)stream);
}

// Features handed in in the caller's row order -> plan (Z-order) row order: out[i] = features[input_index[i]]
API int egonn_gather_input(egonn_ctx* c, const float* features, int channels, float* out, void* stream) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(features && out && channels >= 1, EGONN_ERR_INVALID, "gather_input: bad argument");
  HIP_CHECK(hipSetDevice(c->device));
  EGONN_REQUIRE(!c->from_points, EGONN_ERR_STATE, "gather_input: voxelize plans have no caller row order");
  return gather_rows(features, c->plan.perm0, c->plan.lv[0].n, channels, out, (hipStream_t)stream);
}

// GeM pooling over the rows of level `level` (layers/pooling.py:82-86): out (B, channels)
API int egonn_gem(egonn_ctx* c, int level, const float* x, int channels, const float* p, float* out, void* stream) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS && x && p && out, EGONN_ERR_INVALID, "gem: bad argument");
  HIP_CHECK(hipSetDevice(c->device));
  return op_pool(c, POOL_GEM, level, x, channels, p, out, stream);
}

// MAC pooling over the rows of level `level` (MinkowskiGlobalMaxPooling, layers/pooling.py:46-56): out (B, channels)
API int egonn_global_max_pool(egonn_ctx* c, int level, const float* in, int channels, float* out, void* stream) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS && in && out, EGONN_ERR_INVALID, "global_max_pool: bad argument");
  HIP_CHECK(hipSetDevice(c->device));
  return op_pool(c, POOL_MAC, level, in, channels, nullptr, out, stream);
}

// NetVLAD / NetVLAD-GC pooling over the rows of level `level` (layers/netvlad.py:18-112, netvlad.hip): out (B, out_dim)
API int egonn_netvlad(egonn_ctx* c, int level, const float* x, int channels, const float* cluster_weights,
                      const float* cluster_weights2, const float* bn1_scale, const float* bn1_shift,
                      const float* hidden1_weights, const float* bn2_scale, const float* bn2_shift,
                      const float* gating_weights, const float* gate_scale, const float* gate_shift, int out_dim, int gating,
                      float* out, void* stream) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS, EGONN_ERR_INVALID, "netvlad: level %d out of range", level);
  EGONN_REQUIRE(channels >= 16 && channels <= 512 && channels % 16 == 0, EGONN_ERR_INVALID,
                "netvlad: %d channels unsupported (multiple of 16, 16..512)", channels);
  EGONN_REQUIRE(out_dim >= 16 && out_dim <= 1024 && out_dim % 16 == 0, EGONN_ERR_INVALID,
                "netvlad: output_dim %d unsupported (multiple of 16, 16..1024)", out_dim);
  EGONN_REQUIRE(x && cluster_weights && cluster_weights2 && bn1_scale && bn1_shift && hidden1_weights && bn2_scale &&
                    bn2_shift && out && (gating == 0 || gating == 1),
                EGONN_ERR_INVALID, "netvlad: bad argument");
  EGONN_REQUIRE(!gating || (gating_weights && gate_scale && gate_shift), EGONN_ERR_INVALID,
                "netvlad: gating needs gating_weights and the folded gate BatchNorm");
  EGONN_REQUIRE(((uintptr_t)x & 15) == 0, EGONN_ERR_INVALID, "netvlad: x must be 16-byte aligned");
  HIP_CHECK(hipSetDevice(c->device));
  const int B = c->plan.batch;
  const size_t nws = netvlad_workspace_floats(B, channels, out_dim);
  Arena* A;
  EGONN_TRY(claim_work(c, nws * 4 + 4096, false, &A));
  WALLOC(float, ws, nws);
  return netvlad_forward(x, c->plan.lv[level].boff, B, channels, cluster_weights, cluster_weights2, bn1_scale, bn1_shift,
                         hidden1_weights, out_dim, bn2_scale, bn2_shift, gating_weights, gate_scale, gate_shift, gating, out,
                         ws, (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ model
API int egonn_model_create(egonn_model** m) {
  EGONN_REQUIRE(m, EGONN_ERR_INVALID, "model_create: null out pointer");
  *m = new egonn_model();
  return EGONN_OK;
}

API void egonn_model_destroy(egonn_model* m) {
  if (!m) return;
  m->store.release();
  if (m->conv0_unit) (void)hipFree(m->conv0_unit);
  if (m->lh_pack) (void)hipFree(m->lh_pack);
  if (m->lh_ptrs) (void)hipFree(m->lh_ptrs);
  if (m->fpn) minkfpn_model_free(m->fpn);
  delete m;
}

API int egonn_model_set_tensor(egonn_model* m, const char* key, const float* data, int ndim, const int64_t* shape) {
  EGONN_REQUIRE(m && key && data && ndim >= 0 && ndim <= 4, EGONN_ERR_INVALID, "model_set_tensor: bad argument");
  TensorRef r;
  r.p = data;
  r.shape.assign(shape, shape + ndim);
  m->t[key] = r;
  m->ready = false;
  if (m->fpn) minkfpn_model_invalidate(m->fpn);
  return EGONN_OK;
}

namespace egonn {

int get_tensor(egonn_model* m, const std::string& key, std::initializer_list<int64_t> want, const float** out) {
  auto it = m->t.find(key);
  EGONN_REQUIRE(it != m->t.end(), EGONN_ERR_STATE, "model: missing state_dict tensor '%s'", key.c_str());
  const std::vector<int64_t>& s = it->second.shape;
  bool ok = s.size() == want.size();
  size_t i = 0;
  for (int64_t w : want) {
    if (ok && s[i] != w) ok = false;
    ++i;
  }
  if (!ok) {
    std::string got = "(", exp = "(";
    for (int64_t v : s) got += std::to_string(v) + ",";
    for (int64_t v : want) exp += std::to_string(v) + ",";
    set_error("model: tensor '%s' has shape %s), expected %s)", key.c_str(), got.c_str(), exp.c_str());
    return EGONN_ERR_INVALID;
  }
  *out = it->second.p;
  return EGONN_OK;
}

int get_bn(egonn_model* m, const std::string& prefix, int c, BnRef* bn, ModelStore* store) {
  bn->c = c;
  EGONN_TRY(get_tensor(m, prefix + ".bn.weight", {c}, &bn->w));
  EGONN_TRY(get_tensor(m, prefix + ".bn.bias", {c}, &bn->b));
  EGONN_TRY(get_tensor(m, prefix + ".bn.running_mean", {c}, &bn->rm));
  EGONN_TRY(get_tensor(m, prefix + ".bn.running_var", {c}, &bn->rv));
  store->add_bn(bn);
  return EGONN_OK;
}

int eca_ksize(int c) {
  int lg = 0;
  while ((1 << lg) < c) ++lg;
  const int t = (lg + 1) / 2;
  return (t % 2) ? t : t + 1;
}

int get_block(egonn_model* m, const std::string& prefix, int ci, int co, bool eca, BlockRef* b, ModelStore* store) {
  *b = BlockRef();
  b->cin = ci;
  b->cout = co;
  EGONN_TRY(get_tensor(m, prefix + ".conv1.kernel", {27, ci, co}, &b->conv1));
  EGONN_TRY(get_bn(m, prefix + ".norm1", co, &b->n1, store));
  EGONN_TRY(get_tensor(m, prefix + ".conv2.kernel", {27, co, co}, &b->conv2));
  EGONN_TRY(get_bn(m, prefix + ".norm2", co, &b->n2, store));
  if (ci != co) {
    EGONN_TRY(get_tensor(m, prefix + ".downsample.0.kernel", {ci, co}, &b->down));
    EGONN_TRY(get_bn(m, prefix + ".downsample.1", co, &b->dn, store));
  }
  if (eca) {
    b->eca_k = eca_ksize(co);
    EGONN_TRY(get_tensor(m, prefix + ".eca.conv.weight", {1, 1, b->eca_k}, &b->eca));
  }
  return EGONN_OK;
}

void ModelStore::begin() {
  bns.clear();
  packs.clear();
  bn_bytes = pack_bytes = 0;
}
void ModelStore::add_bn(BnRef* bn) {
  bns.push_back(bn);
  bn_bytes += align_up((size_t)2 * bn->c * sizeof(float), 256);
}
void ModelStore::add_pack(Form form, const float* w, int K, int ci, int co, const void** dst) {
  packs.push_back({form, w, K, ci, co, pack_bytes, dst});
  const size_t n = (size_t)K * ci * co;
  pack_bytes += align_up(form == SPLIT ? split_weights_bytes(K, ci, co) : form == RG16 ? n * 2 : n * 4, 256);
}
void ModelStore::add_kernel(const float* w, int K, int ci, int co, bool bf16, PackedKernel* dst) {
  *dst = PackedKernel();
  add_pack(RG32, w, K, ci, co, &dst->rg32);
  if (bf16) add_pack(RG16, w, K, ci, co, &dst->rg16);
  if (sconv_split_supported(ci, co)) add_pack(SPLIT, w, K, ci, co, &dst->split);
}
int ModelStore::commit(hipStream_t st) {
  auto grow = [](char** buf, size_t* cap, size_t need) -> int {
    if (*cap >= need) return EGONN_OK;
    if (*buf) HIP_CHECK(hipFree(*buf));
    *buf = nullptr;
    *cap = 0;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(buf), need));
    *cap = need;
    return EGONN_OK;
  };
  EGONN_TRY(grow(&folded, &folded_cap, bn_bytes));
  EGONN_TRY(grow(&packed, &packed_cap, pack_bytes));
  for (const Pack& k : packs) {
    char* out = packed + k.off;
    switch (k.form) {
      case RG32: EGONN_TRY(pack_rg_weights(k.w, k.K, k.ci, k.co, 0, 0, 0, out, st)); break;
      case RG16: EGONN_TRY(pack_rg_weights(k.w, k.K, k.ci, k.co, 1, 0, 0, out, st)); break;
      case SPLIT: EGONN_TRY(pack_split_weights(k.w, k.K, k.ci, k.co, 0, 0, out, st)); break;
      case DENSE: EGONN_TRY(dense_pack_frags(k.w, 0, k.ci, k.co, reinterpret_cast<float*>(out), st)); break;
      case DENSE_OI: EGONN_TRY(dense_pack_frags(k.w, 1, k.ci, k.co, reinterpret_cast<float*>(out), st)); break;
    }
    *k.dst = out;
  }
  char* cur = folded;
  for (BnRef* bn : bns) {   // eval-mode BatchNorm folded to scale / shift, eps of nn.BatchNorm1d
    bn->scale = reinterpret_cast<float*>(cur);
    bn->shift = bn->scale + bn->c;
    cur += align_up((size_t)2 * bn->c * sizeof(float), 256);
    EGONN_TRY(bn_fold(bn->w, bn->b, bn->rm, bn->rv, 1e-5f, bn->c, bn->scale, bn->shift, st));
  }
  return EGONN_OK;
}
void ModelStore::release() {
  if (folded) (void)hipFree(folded);
  if (packed) (void)hipFree(packed);
  folded = packed = nullptr;
  folded_cap = packed_cap = 0;
}

}  // namespace egonn

namespace {

int get_mlp(egonn_model* m, const std::string& prefix, int cin, int mid, int cout, MlpRef* r) {
  r->cin = cin; r->mid = mid; r->cout = cout;
  EGONN_TRY(get_tensor(m, prefix + ".net.0.linear.weight", {mid, cin}, &r->w0));
  EGONN_TRY(get_tensor(m, prefix + ".net.0.linear.bias", {mid}, &r->b0));
  EGONN_TRY(get_tensor(m, prefix + ".net.2.linear.weight", {cout, mid}, &r->w1));
  EGONN_TRY(get_tensor(m, prefix + ".net.2.linear.bias", {cout}, &r->b1));
  return EGONN_OK;
}

}  // namespace

API int egonn_model_finalize(egonn_model* m, void* stream) {
  EGONN_REQUIRE(m, EGONN_ERR_INVALID, "model_finalize: null model");
  hipStream_t st = (hipStream_t)stream;
  ModelStore& S = m->store;
  S.begin();
  // ---- resolve every tensor (shapes checked, the offending key named) and register what the store folds and packs: every
  // sparse-conv kernel in item-major MFMA fragment order (sconv.hip), fp32, bf16 and split; the 1x1 kernels the forward runs
  // through the streaming dense kernel, the global head's lateral 1x1 kernels and its decoder's two Linear kernels in the dense
  // kernels' fragment order (fp32 only).  No device work before the last lookup.
  auto dense = [&](const float* w, int ci, int co, const void** dst, ModelStore::Form form = ModelStore::DENSE) {
    *dst = nullptr;
    if (ci % 16 == 0 && co % 16 == 0) S.add_pack(form, w, 1, ci, co, dst);
  };
  EGONN_TRY(get_tensor(m, "trunk.convs.0.kernel", {125, 1, 32}, &m->conv0));
  EGONN_TRY(get_bn(m, "trunk.bn.0", 32, &m->bn[0], &S));
  int inpl = PLANES[0];
  for (int i = 1; i <= 7; ++i) {
    const std::string si = std::to_string(i);
    const int cout = PLANES[i - 1];
    EGONN_TRY(get_tensor(m, "trunk.convs." + si + ".kernel", {8, inpl, inpl}, &m->convs[i]));
    EGONN_TRY(get_bn(m, "trunk.bn." + si, inpl, &m->bn[i], &S));
    BlockRef& b = m->blk[i];
    EGONN_TRY(get_block(m, "trunk.blocks." + si + ".0", inpl, cout, true, &b, &S));
    S.add_kernel(m->convs[i], 8, inpl, inpl, true, &m->pk_convs[i]);
    S.add_kernel(b.conv1, 27, inpl, cout, true, &m->pk_c1[i]);
    S.add_kernel(b.conv2, 27, cout, cout, true, &m->pk_c2[i]);
    m->pk_down[i] = nullptr;
    if (b.down) dense(b.down, inpl, cout, &m->pk_down[i]);
    inpl = cout;
  }
  for (int l : {5, 6, 7}) {
    EGONN_TRY(get_tensor(m, "global_head.conv1x1." + std::to_string(l) + ".kernel", {PLANES[l - 1], GLOBAL_CH}, &m->g1x1[l]));
    dense(m->g1x1[l], PLANES[l - 1], GLOBAL_CH, &m->pk_g1x1[l]);
  }
  for (int l : {6, 7}) {
    EGONN_TRY(get_tensor(m, "global_head.tconv." + std::to_string(l) + ".kernel", {8, GLOBAL_CH, GLOBAL_CH}, &m->gt[l]));
    S.add_kernel(m->gt[l], 8, GLOBAL_CH, GLOBAL_CH, true, &m->pk_gt[l]);
  }
  for (int l : {3, 4}) {
    EGONN_TRY(get_tensor(m, "local_head.conv1x1." + std::to_string(l) + ".kernel", {PLANES[l - 1], LOCAL_CH}, &m->l1x1[l]));
    dense(m->l1x1[l], PLANES[l - 1], LOCAL_CH, &m->pk_l1x1[l]);
  }
  EGONN_TRY(get_tensor(m, "local_head.tconv.4.kernel", {8, LOCAL_CH, LOCAL_CH}, &m->lt[4]));
  S.add_kernel(m->lt[4], 8, LOCAL_CH, LOCAL_CH, true, &m->pk_lt[4]);
  m->gem_p = nullptr;                  // GeM exponent; MAC / SPoC pooling (layers/pooling.py:46-69) has no parameter
  if (m->t.count("global_pooling.pooling.p")) EGONN_TRY(get_tensor(m, "global_pooling.pooling.p", {1}, &m->gem_p));
  EGONN_TRY(get_mlp(m, "global_descriptor_decoder", GLOBAL_CH, GLOBAL_DIM + (GLOBAL_CH - GLOBAL_DIM) / 2, GLOBAL_DIM, &m->gdec));
  m->pk_gdec[0] = m->pk_gdec[1] = nullptr;
  if (global_tail_fusable(m->gdec)) {      // the fused tail of the global head reads both Linear kernels in fragment order
    dense(m->gdec.w0, m->gdec.cin, m->gdec.mid, &m->pk_gdec[0], ModelStore::DENSE_OI);
    dense(m->gdec.w1, m->gdec.mid, m->gdec.cout, &m->pk_gdec[1], ModelStore::DENSE_OI);
  }
  EGONN_TRY(get_mlp(m, "local_descriptor_decoder", LOCAL_CH, LOCAL_DIM + (LOCAL_CH - LOCAL_DIM) / 2, LOCAL_DIM, &m->ldec));
  EGONN_TRY(get_mlp(m, "local_keypoint_regressor", LOCAL_CH, LOCAL_CH / 2, 3, &m->kp));
  EGONN_TRY(get_mlp(m, "local_sigma_regressor", LOCAL_CH, LOCAL_CH / 2, 1, &m->sg));

  // ---- device work from here on
  EGONN_TRY(S.commit(st));
  if (!m->conv0_unit) HIP_CHECK(hipMalloc(&m->conv0_unit, 2 * 4 * 3 * 64 * 16));
  EGONN_TRY(conv0_pack_unit(m->conv0, m->conv0_unit, st));
  if (m->ldec.cin == 64 && m->ldec.mid == 96 && m->ldec.cout == 128 && m->kp.mid == 32 && m->sg.mid == 32 && m->kp.cin == 64 &&
      m->sg.cin == 64) {       // the local heads of models/minkgl.py:175-225 in their shipped sizes: split-fp16 fragments
    if (!m->lh_pack) HIP_CHECK(hipMalloc(&m->lh_pack, local_heads_pack_bytes()));
    if (!m->lh_ptrs) HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&m->lh_ptrs), 6 * sizeof(float*)));
    const float* hp[6] = {m->ldec.w0, m->ldec.w1, m->kp.w0, m->kp.w1, m->sg.w0, m->sg.w1};
    HIP_CHECK(hipMemcpyAsync(m->lh_ptrs, hp, sizeof(hp), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipStreamSynchronize(st));                    // (hp lives on this stack frame)
    EGONN_TRY(local_heads_pack(m->lh_ptrs, m->lh_pack, st));
  }
  m->ready = true;
  return EGONN_OK;
}

// ------------------------------------------------------------------------------------------ forward
namespace {

int run_mlp(const MlpRef& r, const float* x, int64_t n, int act_out, float* hidden, float* out, hipStream_t st,
            const int32_t* n_dev) {
  EGONN_TRY(dense_forward({.in = x, .n = n, .n_dev = n_dev, .cin = r.cin, .cout = r.mid, .W = r.w0, .w_out_in = 1, .bias = r.b0,
                           .act = ACT_RELU, .out = hidden},
                          st));
  return dense_forward({.in = hidden, .n = n, .n_dev = n_dev, .cin = r.mid, .cout = r.cout, .W = r.w1, .w_out_in = 1, .bias = r.b1,
                        .act = act_out, .out = out},
                       st);
}

}  // namespace

namespace egonn {

int claim_work(egonn_ctx* c, size_t bytes, bool with_ksplit, Arena** A) {
  for (int l = 0; l < EGONN_NUM_LEVELS; ++l) c->level_feat[l] = nullptr;
  c->ks_part = nullptr;
  c->ks_part_floats = 0;
  EGONN_TRY(c->work_arena.ensure(bytes));
  c->work_arena.reset();
  *A = &c->work_arena;
  // partial tiles of the offset-split launches: ONE buffer, written by a convolution and consumed by its reducer before the
  // next launch of the same stream writes it again
  const size_t ks = with_ksplit ? sconv_ksplit_scratch_floats(c) : 0;
  if (ks) {
    c->ks_part = (*A)->alloc<float>(ks);
    EGONN_REQUIRE(c->ks_part, EGONN_ERR_STATE, "work arena too small (ks_part)");
    c->ks_part_floats = ks;
  }
  return EGONN_OK;
}

// One sparse convolution of the graph: the profiler tag "<kernel><cin,cout>/L<level>/<what>" (the kernel sconv_map will dispatch,
// so that bench.py's roofline leg names what rocprofv3 names), the timing scope, the launch
int conv_layer(egonn_ctx* c, hipStream_t st, const ConvCall& cc, const char* what) {
  static const int pk[3] = {PK_K3, PK_K2S2, PK_TCONV};
  char tag[64];
  snprintf(tag, sizeof(tag), "%s<%d,%d>/L%d/%s", sconv_kernel_name(c, cc.kind, cc.level, cc.cin, cc.cout, cc.bf16), cc.cin, cc.cout,
           cc.level, what);
  ProfScope ps(c, st, tag, pk[cc.kind], cc.level, cc.kind == 0 ? 27 : 8, cc.cin, cc.cout, cc.bf16 ? 2 : 4);
  return sconv_map(c, cc, st);
}
ConvCall conv_call(int kind, int level, const void* in, const PackedKernel& pk, int cin, int cout, int bf16, const BnRef* bn, int relu,
                   void* out) {
  return ConvCall{.kind = kind, .level = level, .in = in, .out = out, .cin = cin, .cout = cout, .bf16 = bf16,
                  .scale = bn ? bn->scale : nullptr, .shift = bn ? bn->shift : nullptr, .relu = relu, .packed = &pk};
}

int ensure_graph_rowgroups(egonn_ctx* c, int L, const int* tlevels, int nt, hipStream_t st) {
  int kinds[RG_MAX_JOBS], levels[RG_MAX_JOBS], n = 0;
  for (int l = 1; l <= L; ++l) { kinds[n] = 0; levels[n++] = l; }
  for (int l = 1; l <= L; ++l) { kinds[n] = 1; levels[n++] = l; }
  for (int i = 0; i < nt; ++i) { kinds[n] = 2; levels[n++] = tlevels[i]; }
  return ensure_rowgroups(c, kinds, levels, n, st);
}

int block_convs(egonn_ctx* c, hipStream_t st, Arena* A, int level, const BlockRef& b, const PackedKernel& pk1, const PackedKernel& pk2,
                int bf16, const void* in, float* psum, void** t2_out) {
  const size_t bytes = (size_t)c->plan.cap[level] * b.cout * (bf16 ? 2 : 4);
  WALLOC(char, t1, bytes);
  WALLOC(char, t2, bytes);
  const bool t1_split = !switches().no_presplit && sconv_route(c, 0, level, b.cin, b.cout, bf16) == ROUTE_SPLIT &&
                        sconv_route(c, 0, level, b.cout, b.cout, bf16) == ROUTE_SPLIT;
  ConvCall c1 = conv_call(0, level, in, pk1, b.cin, b.cout, bf16, &b.n1, 1, t1);
  c1.split_io = t1_split ? 2 : 0;
  EGONN_TRY(conv_layer(c, st, c1, "k3.conv1"));
  ConvCall c2 = conv_call(0, level, t1, pk2, b.cout, b.cout, bf16, &b.n2, 0, t2);
  c2.split_io = t1_split ? 1 : 0;
  c2.psum = psum;
  EGONN_TRY(conv_layer(c, st, c2, "k3.conv2"));
  *t2_out = t2;
  return EGONN_OK;
}

DenseCall down_call(const BlockRef& b, const void* in, int bf16, int64_t n, const int32_t* n_dev, const void* wfrag) {
  return DenseCall{.in = in, .in_bf16 = bf16, .n = n, .n_dev = n_dev, .cin = b.cin, .cout = b.cout, .W = b.down,
                   .wfrag = static_cast<const float*>(wfrag), .scale = b.dn.scale, .shift = b.dn.shift, .out_bf16 = bf16};
}

// pow_mode of the partial sums: GeM = sum of clamp(x)^p (layers/pooling.py:72-86), MAC = max (:46-56), SPoC = average (:59-69)
static int pool_pow_mode(Pooling method) { return method == POOL_GEM ? 1 : method == POOL_MAC ? 2 : 0; }
static int global_pool_finish(Pooling method, const float* partial, const int32_t* boff, int B, int C, const float* p, float* out,
                              hipStream_t st) {
  if (method == POOL_GEM) return gem_finish(partial, boff, B, C, p, out, st);
  return pool_finish(partial, boff, B, C, pool_pow_mode(method), out, st);
}
int global_pool(Pooling method, const float* x, const int32_t* boff, int B, int C, const float* p, float* partial, float* out,
                hipStream_t st) {
  EGONN_TRY(segment_partial_sums(x, boff, B, C, pool_pow_mode(method), method == POOL_GEM ? p : nullptr, partial, st));
  return global_pool_finish(method, partial, boff, B, C, p, out, st);
}

bool global_tail_fusable(const MlpRef& r) { return r.cin == GTAIL_CIN && r.mid == GTAIL_MID && r.cout == GTAIL_OUT; }
int global_tail(const MlpRef& r, const void* const* pk, const float* g5, int64_t ncap, const int32_t* n_dev, const int32_t* boff, int B,
                Pooling method, const float* p, bool fused, float* gh, float* gd, float* partial, float* out, hipStream_t st) {
  if (fused) {
    EGONN_REQUIRE(global_tail_fusable(r) && pk && pk[0] && pk[1], EGONN_ERR_STATE, "global tail: no fused form for %d->%d->%d", r.cin,
                  r.mid, r.cout);
    EGONN_TRY(global_tail_fused(g5, ncap, boff, B, static_cast<const float*>(pk[0]), r.b0, static_cast<const float*>(pk[1]), r.b1,
                                pool_pow_mode(method), method == POOL_GEM ? p : nullptr, partial, st));
    return global_pool_finish(method, partial, boff, B, r.cout, p, out, st);
  }
  EGONN_TRY(run_mlp(r, g5, ncap, ACT_NONE, gh, gd, st, n_dev));
  return global_pool(method, gd, boff, B, r.cout, p, partial, out, st);
}

int block_tail(const float* x, const float* res, const int32_t* boff, int B, int64_t n, int ch, const float* eca, int eca_k,
               float* partial, float* out, hipStream_t st) {
  if (!eca) return add_act(x, res, n * ch, 1, out, st);
  EGONN_TRY(segment_partial_sums(x, boff, B, ch, 0, nullptr, partial, st));
  return eca_apply(x, res, partial, boff, B, n, ch, eca, eca_k, out, st);
}

}  // namespace egonn

API int egonn_forward(egonn_ctx* c, egonn_model* m, const float* features, int quant_mode, const float* step, int flags,
                      float* out_global, float* out_desc, float* out_kp, float* out_sigma, void* stream) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(m && m->ready, EGONN_ERR_STATE, "model not finalized (call egonn_model_finalize)");
  EGONN_REQUIRE(step, EGONN_ERR_INVALID, "forward: null argument");
  HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  Plan& P = c->plan;
  const int B = P.batch;
  const int32_t* cnt = c->dev_counts;                          // device row counts per level (the kernels clip to them)
  const int bf16 = (flags & EGONN_FLAG_BF16) ? 1 : 0;          // feature maps + sparse-conv weights in bf16 (configs[2])
  const size_t es = bf16 ? 2 : 4;                              // bytes per feature-map element
  const bool do_global = !(flags & EGONN_FLAG_DISABLE_GLOBAL);
  const bool do_local = !(flags & EGONN_FLAG_DISABLE_LOCAL);
  EGONN_REQUIRE(!do_global || out_global, EGONN_ERR_INVALID, "forward: out_global is null");
  EGONN_REQUIRE(!do_local || (out_desc && out_kp && out_sigma), EGONN_ERR_INVALID, "forward: local outputs are null");
  // the fp16 range flag covers THIS forward: cleared in stream order (a memset node of a captured graph), so a status read after
  // it reports this batch and not an earlier forward on the same plan; the plan's coordinate / capacity bits are another word
  HIP_CHECK(hipMemsetAsync(c->dev_fp16_flag, 0, sizeof(int32_t), st));

  // ---- row-group tables of every map the graph uses: one launch per plan
  {
    const int tlevels[3] = {6, 5, 3};      // the global head's transposed maps, the local head's
    EGONN_TRY(ensure_graph_rowgroups(c, 7, tlevels + (do_global ? 0 : 2), (do_global ? 2 : 0) + (do_local ? 1 : 0), st));
    DBG_SYNC("row groups");
  }

  // ---- workspace: every intermediate gets its own buffer (HBM is plentiful; no aliasing hazards)
  size_t need = (size_t)P.cap[0] * (1 + 32) * 4;
  for (int i = 1; i <= 7; ++i) need += (size_t)P.cap[i] * 128 * 4 * 6 + (size_t)P.lv[i].rg27.cap_groups * 128 * 4;
  need += (size_t)P.cap[5] * (192 + 256 + 128 * 2) * 4 + (size_t)P.cap[3] * (96 + 32 + 32 + 3 + 64 * 2) * 4;
  need += (size_t)B * SEG_CHUNKS * 256 * 4 * 10 + (size_t)P.cap[3] * 32 + (4u << 20);
  need += sconv_ksplit_scratch_floats(c) * 4 + 4096;
  Arena* A;
  EGONN_TRY(claim_work(c, need, true, &A));

  // ---- trunk (models/minkgl.py:136-153)
  const int64_t n0 = P.cap[0];
  const float* f0 = features;          // voxelize plans: features are already in level-0 row order; NULL = all ones
  if (features && !c->from_points) {
    WALLOC(float, fg, n0);
    EGONN_TRY(gather_rows(features, P.perm0, n0, 1, fg, st, cnt));
    f0 = fg;
  }
  WALLOC(char, x0, n0 * 32 * es);
  {
    ProfScope ps(c, st, "conv0_k5_kernel/L0", PK_CONV0, 0, 125, 1, 32, (int)es);
    EGONN_TRY(conv0_k5_forward(c, f0, m->conv0, 32, m->bn[0].scale, m->bn[0].shift, 1, x0, bf16, st, m->conv0_unit));
  }
  DBG_SYNC("conv0");
  const void* x[8] = {x0};
  c->level_feat[0] = x0;
  c->level_ch[0] = 32;
  c->level_bf16 = bf16;
  // ---- local head, descriptor / keypoint / sigma regressors (models/minkgl.py:287-308)
  auto local_head = [&](hipStream_t st) -> int {
    const int64_t n3 = P.cap[3], n4 = P.cap[4];
    WALLOC(char, l4, n4 * LOCAL_CH * es);
    EGONN_TRY(dense_forward({.in = x[4], .in_bf16 = bf16, .n = n4, .n_dev = cnt + 4, .cin = 128, .cout = LOCAL_CH, .W = m->l1x1[4],
                             .wfrag = static_cast<const float*>(m->pk_l1x1[4]), .out = l4, .out_bf16 = bf16},
                            st));
    WALLOC(char, u3, n3 * LOCAL_CH * es);
    EGONN_TRY(conv_layer(c, st, conv_call(2, 3, l4, m->pk_lt[4], LOCAL_CH, LOCAL_CH, bf16, nullptr, 0, u3), "tconv"));
    EGONN_REQUIRE(m->ldec.cin == 64 && m->ldec.mid == 96 && m->ldec.cout == 128 && m->kp.mid == 32 && m->sg.mid == 32,
                  EGONN_ERR_STATE, "local heads: unexpected layer sizes");
    const float* hw[12] = {m->ldec.w0, m->ldec.b0, m->ldec.w1, m->ldec.b1, m->kp.w0, m->kp.b0, m->kp.w1, m->kp.b1,
                           m->sg.w0, m->sg.b0, m->sg.w1, m->sg.b1};
    // the heads' Linear layers on the fp16 matrix pipe (heads.hip), unless this context asked for exact fp32 arithmetic
    const void* lh_pack = (!switches().no_split_heads && sconv_split_arithmetic(c)) ? m->lh_pack : nullptr;
    if (!switches().no_fused_lateral && LOCAL_CH == 64) {
      // the level-3 lateral 1x1 convolution + the transposed convolution's output are the first layer of the heads' kernel — the
      // 64-channel map they read is never written (bitwise the rows of the dense launch this replaces; bf16 maps are widened on load)
      EGONN_TRY(local_heads_forward(reinterpret_cast<const float*>(x[3]), n3, cnt + 3, hw, P.lv[3].keys, 3, P.coord_bits, quant_mode,
                                    step, (flags & EGONN_FLAG_IGNORE_KP_REGRESSOR) ? 1 : 0, out_desc, out_kp, out_sigma, st,
                                    m->l1x1[3], reinterpret_cast<const float*>(u3), bf16, lh_pack, c->dev_fp16_flag));
      return EGONN_OK;
    }
    WALLOC(float, l3, n3 * LOCAL_CH);
    EGONN_TRY(dense_forward({.in = x[3], .in_bf16 = bf16, .n = n3, .n_dev = cnt + 3, .cin = 64, .cout = LOCAL_CH, .W = m->l1x1[3],
                             .wfrag = static_cast<const float*>(m->pk_l1x1[3]), .residual = u3, .res_bf16 = bf16, .out = l3},
                            st));
    EGONN_TRY(local_heads_forward(l3, n3, cnt + 3, hw, P.lv[3].keys, 3, P.coord_bits, quant_mode, step,
                                  (flags & EGONN_FLAG_IGNORE_KP_REGRESSOR) ? 1 : 0, out_desc, out_kp, out_sigma, st, nullptr, nullptr, 0,
                                  lh_pack, c->dev_fp16_flag));
    return EGONN_OK;
  };
  const float *gated_t2 = nullptr, *gated_res = nullptr, *gated_gate = nullptr;     // level 1's block tail, evaluated by level 2's k=2 conv
  for (int i = 1; i <= 7; ++i) {
    const BlockRef& b = m->blk[i];
    const Level& L = P.lv[i];
    const int64_t n = P.cap[i];
    WALLOC(char, y, n * b.cin * es);
    {
      ConvCall cc = conv_call(1, i, x[i - 1], m->pk_convs[i], b.cin, b.cin, bf16, &m->bn[i], 1, y);
      if (gated_t2 && i == 2) {      // the block output of level 1 is evaluated on the gathered rows — see below
        cc.in = gated_t2;
        cc.in2 = gated_res;
        cc.gate = gated_gate;
      }
      EGONN_TRY(conv_layer(c, st, cc, "k2s2"));
    }
    DBG_SYNC("L%d k2s2", i);
    // ECABasicBlock (layers/eca_block.py:56-73); the gate comes from the column sums conv2's epilogue leaves behind
    WALLOC(float, psum, (size_t)L.rg27.cap_groups * b.cout);
    void* t2 = nullptr;
    EGONN_TRY(block_convs(c, st, A, i, b, m->pk_c1[i], m->pk_c2[i], bf16, y, psum, &t2));
    WALLOC(float, gate, (size_t)B * b.cout);
    DBG_SYNC("L%d convs", i);
    EGONN_TRY(eca_gate_groups(psum, L.rg27, L.boff, B, b.cout, b.eca, b.eca_k, gate, st));
    DBG_SYNC("L%d eca gate", i);
    const void* res = y;
    if (i == 1 && !switches().no_gated_k2s2 && !c->keep_level_features && !bf16 && !b.down && c->sconv.set.product() && b.cout == 32 &&
        m->blk[2].cin == 32 && sconv_route(c, 1, 2, 32, 32, 0) == ROUTE_SPLIT) {
      // level 1's block output has ONE reader, the strided convolution into level 2, which reads every row exactly once: it
      // evaluates relu(t2 * gate[scan] + y) on the rows it gathers (sconv_split_kernel<32,32,...,GATED>) — the 23 MB map is neither
      // written nor read back and the element-wise launch is gone; bitwise the same level-2 input.  egonn_forward_level_features(1)
      // has nothing to return then.
      gated_t2 = reinterpret_cast<const float*>(t2);
      gated_res = reinterpret_cast<const float*>(y);
      gated_gate = gate;
      x[i] = nullptr;
      c->level_feat[i] = nullptr;
      c->level_ch[i] = b.cout;
      continue;
    }
    WALLOC(char, xo, n * b.cout * es);
    // the 1x1 downsample branch with its BatchNorm (levels 2 and 4); its output and what rides on it follow
    const DenseCall down = down_call(b, y, bf16, n, cnt + i, m->pk_down[i]);
    if (b.down && !switches().no_fused_down && dense_gate_fusable(n, b.cin, b.cout)) {
      // blocks with a 1x1 downsample branch (levels 2 and 4): the branch, its BatchNorm and the gated residual + ReLU of the block's
      // tail in ONE launch — out = relu(t2 * gate[scan] + bn(y @ Wd)); the branch output never goes to memory (bitwise the result
      // of the two launches it replaces)
      DenseCall dc = down;
      dc.residual = t2; dc.res_bf16 = bf16;
      dc.gate = gate; dc.boff = L.boff; dc.B = B;
      dc.out = xo;
      EGONN_TRY(dense_forward(dc, st));
    } else {
      if (b.down) {
        WALLOC(char, rd, n * b.cout * es);
        DenseCall dc = down;
        dc.out = rd;
        EGONN_TRY(dense_forward(dc, st));
        res = rd;
      }
      EGONN_TRY(eca_apply_gate(t2, res, gate, L.boff, B, n, b.cout, xo, bf16, st));
    }
    DBG_SYNC("L%d eca apply", i);
    x[i] = xo;
    c->level_feat[i] = xo;
    c->level_ch[i] = b.cout;
    // (measured: forking the local head onto a second stream here — a parallel branch of the captured graph — shortens
    //  one batch by 4 % but costs 28 % throughput with three graphs in flight: multi-branch graphs launch 4x slower and
    //  serialise against each other; the overlap comes from the batches in flight instead)
  }
  if (do_local) EGONN_TRY(local_head(st));
  DBG_SYNC("local head");

  // ---- global head + decoder + GeM (models/minkgl.py:46-60, 207-225; layers/pooling.py:82-86)
  void* g5_fused = nullptr;
  if (do_global && !switches().no_fused_ghead && !bf16 && c->sconv.set.product() && dense_group3_rows(P.cap[5]) &&
      dense_group3_rows(P.cap[6]) && dense_group3_rows(P.cap[7])) {
    // MinkHead (models/minkgl.py:46-60) in three launches instead of five: the three lateral 1x1 convolutions depend on the trunk
    // only — ONE grouped launch — and every FPN step `tconv(y) + lateral` is the transposed convolution with the lateral as its
    // epilogue residual.  a + b = b + a: bitwise the five-launch result (tools/check_bitwise_switches.py).
    WALLOC(float, l7, P.cap[7] * GLOBAL_CH);
    WALLOC(float, l6, P.cap[6] * GLOBAL_CH);
    WALLOC(float, l5, P.cap[5] * GLOBAL_CH);
    WALLOC(float, g6f, P.cap[6] * GLOBAL_CH);
    WALLOC(float, g5f, P.cap[5] * GLOBAL_CH);
    const float* gin[3] = {reinterpret_cast<const float*>(x[7]), reinterpret_cast<const float*>(x[6]), reinterpret_cast<const float*>(x[5])};
    const int64_t gn[3] = {P.cap[7], P.cap[6], P.cap[5]};
    const int32_t* gnd[3] = {cnt + 7, cnt + 6, cnt + 5};
    const float* gw[3] = {m->g1x1[7], m->g1x1[6], m->g1x1[5]};
    float* gout[3] = {l7, l6, l5};
    const float* gpk[3] = {static_cast<const float*>(m->pk_g1x1[7]), static_cast<const float*>(m->pk_g1x1[6]),
                           static_cast<const float*>(m->pk_g1x1[5])};
    EGONN_TRY(dense_small_group3(gin, gn, gnd, gw, switches().no_packed_laterals ? nullptr : gpk, gout, st));
    for (int lv = 6; lv >= 5; --lv) {
      ConvCall cc = conv_call(2, lv, lv == 6 ? l7 : g6f, m->pk_gt[lv + 1], GLOBAL_CH, GLOBAL_CH, 0, nullptr, 0, lv == 6 ? g6f : g5f);
      cc.residual = lv == 6 ? l6 : l5;
      EGONN_TRY(conv_layer(c, st, cc, "tconv"));
    }
    g5_fused = g5f;
    DBG_SYNC("global head (fused)");
  }
  if (do_global) {
    const float* g5 = reinterpret_cast<const float*>(g5_fused);
    if (!g5) {
    // lateral 1x1 convolution of level l (+ the transposed convolution's output as its residual)
    auto lateral = [&](int l, const void* up, void* out, int out_bf16) {
      return dense_forward({.in = x[l], .in_bf16 = bf16, .n = P.cap[l], .n_dev = cnt + l, .cin = 128, .cout = GLOBAL_CH, .W = m->g1x1[l],
                            .residual = up, .res_bf16 = up ? bf16 : 0, .out = out, .out_bf16 = out_bf16},
                           st);
    };
    WALLOC(char, g7, P.cap[7] * GLOBAL_CH * es);
    EGONN_TRY(lateral(7, nullptr, g7, bf16));
    WALLOC(char, u6, P.cap[6] * GLOBAL_CH * es);
    EGONN_TRY(conv_layer(c, st, conv_call(2, 6, g7, m->pk_gt[7], GLOBAL_CH, GLOBAL_CH, bf16, nullptr, 0, u6), "tconv"));
    WALLOC(char, g6, P.cap[6] * GLOBAL_CH * es);
    EGONN_TRY(lateral(6, u6, g6, bf16));
    WALLOC(char, u5, P.cap[5] * GLOBAL_CH * es);
    EGONN_TRY(conv_layer(c, st, conv_call(2, 5, g6, m->pk_gt[6], GLOBAL_CH, GLOBAL_CH, bf16, nullptr, 0, u5), "tconv"));
    WALLOC(float, g5u, P.cap[5] * GLOBAL_CH);
    EGONN_TRY(lateral(5, u5, g5u, 0));
    g5 = g5u;
    DBG_SYNC("global head");
    }
    WALLOC(float, gh, P.cap[5] * m->gdec.mid);
    WALLOC(float, gd, P.cap[5] * GLOBAL_DIM);
    WALLOC(float, gp, (size_t)B * SEG_CHUNKS * GLOBAL_DIM);
    // global pooling (layers/pooling.py:13-43): GeM (default, :72-86), SPoC = average (:59-69), MAC = max (:46-56)
    const Pooling pool = (flags & EGONN_FLAG_POOL_MAC) ? POOL_MAC : (flags & EGONN_FLAG_POOL_SPOC) ? POOL_SPOC : POOL_GEM;
    EGONN_REQUIRE(pool != POOL_GEM || m->gem_p, EGONN_ERR_STATE, "forward: GeM pooling needs the tensor 'global_pooling.pooling.p'");
    // decoder + partial sums in ONE launch when the decoder has its shipped sizes (g5 is fp32 for both map precisions): the hidden
    // map and the decoder output are never written; bitwise the partial sums of the three launches (tests/test_gpu_global_tail.py)
    const bool fused_tail = !switches().no_fused_gtail && global_tail_fusable(m->gdec) && m->pk_gdec[0] && m->pk_gdec[1];
    EGONN_TRY(global_tail(m->gdec, m->pk_gdec, g5, P.cap[5], cnt + 5, P.lv[5].boff, B, pool, m->gem_p, fused_tail, gh, gd, gp, out_global, st));
  }

  DBG_SYNC("global decoder + pooling");
  return EGONN_OK;
}

// ------------------------------------------------------------------ test hook (tests/test_gpu_global_tail.py; no product path calls it)
// global_tail on the caller's rows and decoder, without a context or a model: scratch = hidden map | decoder output | the two
// kernels in fragment order
static size_t debug_tail_span(int64_t ncap) {
  return align_up((size_t)ncap * GTAIL_MID * 4, 256) + align_up((size_t)ncap * GTAIL_OUT * 4, 256) +
         align_up((size_t)GTAIL_CIN * GTAIL_MID * 4, 256) + align_up((size_t)GTAIL_MID * GTAIL_OUT * 4, 256) + 1024;
}
API int64_t egonn_debug_global_tail_scratch_bytes(int64_t rows_capacity) {
  if (rows_capacity < 0 || rows_capacity >= (1ll << 31) / GTAIL_OUT) return -1;
  return (int64_t)debug_tail_span(rows_capacity);
}
API int egonn_debug_global_tail(const float* g5, const int32_t* row_offsets, int batch_size, int64_t rows_capacity, const int32_t* n_dev,
                                const float* w0, const float* b0, const float* w1, const float* b1, const float* p, int pooling, int form,
                                float* partial, float* out, void* scratch, int64_t scratch_bytes, void* stream) {
  EGONN_REQUIRE(g5 && row_offsets && n_dev && w0 && b0 && w1 && b1 && partial && out && scratch, EGONN_ERR_INVALID,
                "debug_global_tail: null pointer");
  EGONN_REQUIRE(batch_size >= 1 && batch_size <= EGONN_MAX_BATCH, EGONN_ERR_INVALID, "debug_global_tail: batch_size=%d outside [1, %d]",
                batch_size, EGONN_MAX_BATCH);
  EGONN_REQUIRE(rows_capacity >= 0 && rows_capacity < (1ll << 31) / GTAIL_OUT, EGONN_ERR_INVALID,
                "debug_global_tail: rows_capacity=%lld outside [0, 2^31 / %d)", (long long)rows_capacity, GTAIL_OUT);
  EGONN_REQUIRE(pooling >= POOL_GEM && pooling <= POOL_SPOC && (pooling != POOL_GEM || p), EGONN_ERR_INVALID,
                "debug_global_tail: pooling=%d (1 GeM with its exponent, 2 MAC, 3 SPoC)", pooling);
  EGONN_REQUIRE(form == 0 || form == 1, EGONN_ERR_INVALID, "debug_global_tail: form=%d (0 three launches, 1 the fused launch)", form);
  const size_t need = debug_tail_span(rows_capacity);
  EGONN_REQUIRE(scratch_bytes >= (int64_t)need && ((uintptr_t)scratch & 255) == 0, EGONN_ERR_INVALID,
                "debug_global_tail: scratch needs %lld bytes, 256-byte aligned", (long long)need);
  hipStream_t st = (hipStream_t)stream;
  Arena ws = Arena::view(scratch, need);
  float* gh = ws.alloc<float>((size_t)rows_capacity * GTAIL_MID);
  float* gd = ws.alloc<float>((size_t)rows_capacity * GTAIL_OUT);
  float* pk0 = ws.alloc<float>((size_t)GTAIL_CIN * GTAIL_MID);
  float* pk1 = ws.alloc<float>((size_t)GTAIL_MID * GTAIL_OUT);
  EGONN_REQUIRE(gh && gd && pk0 && pk1, EGONN_ERR_STATE, "debug_global_tail: scratch span too small");
  const MlpRef r{.w0 = w0, .b0 = b0, .w1 = w1, .b1 = b1, .cin = GTAIL_CIN, .mid = GTAIL_MID, .cout = GTAIL_OUT};
  const void* pk[2] = {pk0, pk1};
  if (form == 1) {
    EGONN_TRY(dense_pack_frags(w0, 1, r.cin, r.mid, pk0, st));
    EGONN_TRY(dense_pack_frags(w1, 1, r.mid, r.cout, pk1, st));
  }
  return global_tail(r, pk, g5, rows_capacity, n_dev, row_offsets, batch_size, (Pooling)pooling, p, form == 1, gh, gd, partial, out, st);
}

API int egonn_forward_level_features(egonn_ctx* c, int level, float* out, int channels, void* stream) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(level >= 0 && level < EGONN_NUM_LEVELS && c->level_feat[level], EGONN_ERR_STATE,
                "no features for level %d (run egonn_forward first; level 1 of fp32 maps is materialised only after "
                "egonn_debug_keep_level_features(ctx, 1))", level);
  EGONN_REQUIRE(channels == c->level_ch[level], EGONN_ERR_INVALID, "level %d has %d channels, caller expects %d", level,
                c->level_ch[level], channels);
  const int64_t cnt = c->plan.lv[level].n * channels;
  if (c->level_bf16) return convert_bf16_to_f32(c->level_feat[level], cnt, out, (hipStream_t)stream);
  HIP_CHECK(hipMemcpyAsync(out, c->level_feat[level], sizeof(float) * cnt, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return EGONN_OK;
}

API int egonn_select_keypoints(egonn_ctx* c, const float* sigma, const float* keypoints, const float* descriptors,
                               int n_k, float* sel_kp, float* sel_desc, int32_t* sel_rows, int32_t* sel_count,
                               void* stream) {
  REQUIRE_PLAN(c);
  EGONN_REQUIRE(sigma && keypoints && descriptors && sel_kp && sel_desc && sel_rows && sel_count, EGONN_ERR_INVALID,
                "select_keypoints: null argument");
  HIP_CHECK(hipSetDevice(c->device));
  return select_topk(sigma, c->plan.lv[3].boff, c->plan.batch, n_k, keypoints, descriptors, LOCAL_DIM, sel_rows, sel_count,
                     sel_kp, sel_desc, (hipStream_t)stream);
}


// torch.topk(sigma, n_k, largest=False) per segment (eval/evaluate.py:359) without a plan: row_offsets DEVICE int32 (B+1)
API int egonn_topk_rows(const float* sigma, const int32_t* row_offsets, int batch_size, int n_k, int32_t* sel_rows,
                        int32_t* sel_count, void* stream) {
  EGONN_REQUIRE(sigma && row_offsets && sel_rows && sel_count && batch_size >= 1, EGONN_ERR_INVALID, "topk_rows: bad argument");
  return select_topk(sigma, row_offsets, batch_size, n_k, nullptr, nullptr, 0, sel_rows, sel_count, nullptr, nullptr,
                     (hipStream_t)stream);
}

// ------------------------------------------------------------------------------------------ launch timing (bench.py)
API int egonn_profile_enable(egonn_ctx* c, int mode, const char* filter) {
  EGONN_REQUIRE(c && mode >= 0 && mode <= 3, EGONN_ERR_INVALID, "profile_enable: bad argument");
  c->prof.mode = mode;
  snprintf(c->prof.filter, sizeof(c->prof.filter), "%s", filter ? filter : "");
  return EGONN_OK;
}

// Drains the timing records collected since the last fetch.  [SYNC]  Returns up to `cap` records:
// names (cap x 64 chars), milliseconds, algorithmic bytes (P*Cin*e + N_out*Cout*e + K*Cin*Cout*e + 8*P; e = 4 fp32 / 2 bf16) and flops
// (2*P*Cin*Cout) of every launch; *n = number of records written.
API int egonn_profile_fetch(egonn_ctx* c, int cap, int* n, char* names, float* ms, double* bytes, double* flops,
                            void* stream) {
  EGONN_REQUIRE(c && n && names && ms && bytes && flops, EGONN_ERR_INVALID, "profile_fetch: null argument");
  HIP_CHECK(hipSetDevice(c->device));
  Plan& P = c->plan;
  if (P.valid) {
    if (P.built_reserved) P.exact = false;      // replays rebuilt the plan: read this batch's sizes
    EGONN_TRY(plan_sync(c, (hipStream_t)stream));
    EGONN_TRY(count_map_pairs(c, (hipStream_t)stream));   // [0] = first-layer pairs, [l] = k=3 map of level l
  }
  HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  unsigned long long pairs[16];
  HIP_CHECK(hipMemcpy(pairs, c->dev_pairs, sizeof(pairs), hipMemcpyDeviceToHost));
  int w = 0;
  std::vector<ProfRec> all(c->prof.recs);
  all.insert(all.end(), c->prof.graph_recs.begin(), c->prof.graph_recs.end());   // the last replay's brackets
  const size_t n_plain = c->prof.recs.size();
  size_t ri = 0;
  for (auto& r : all) {
    const bool plain = ri++ < n_plain;
    float t = 0.f;
    if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&t, r.e0, r.e1) != hipSuccess) {
      (void)hipGetLastError();
      if (plain) { c->prof.pool.push_back(r.e0); c->prof.pool.push_back(r.e1); }
      continue;                                          // an event a replay has not recorded (yet)
    }
    if (w < cap) {
      // output rows and map pairs of the launch, from the plan's true sizes
      const double n_out = (double)P.lv[r.level].n;
      double Pn = 0;
      switch (r.kind) {
        case PK_CONV0: Pn = (double)pairs[0]; break;
        case PK_K3: Pn = (double)pairs[r.level]; break;
        case PK_K2S2: Pn = (double)P.lv[r.level - 1].n; break;      // every input voxel feeds exactly one parent
        case PK_TCONV: Pn = n_out; break;
        default: Pn = n_out; break;
      }
      snprintf(names + (size_t)w * 64, 64, "%s", r.name);
      ms[w] = t;
      bytes[w] = Pn * r.cin * r.es + n_out * r.cout * r.es + (double)r.K * r.cin * r.cout * r.es + 8.0 * Pn;
      flops[w] = 2.0 * Pn * r.cin * r.cout;
      ++w;
    }
    if (plain) { c->prof.pool.push_back(r.e0); c->prof.pool.push_back(r.e1); }
  }
  c->prof.recs.clear();
  *n = w;
  return EGONN_OK;
}
