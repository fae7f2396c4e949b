// The second model kind of the C ABI: MinkFPN + global pooling (MinkLoc / MinkLoc3D) as ONE fixed launch sequence per batch.
//
// The graph restates MinkFPN.forward (reference models/minkfpn.py:65-93: conv0, the bottom-up levels of strided convolution +
// residual blocks — ME BasicBlock or ECABasicBlock, layers/eca_block.py:56-73 — the 1x1 convolution of the coarsest level and the
// top-down steps `tconv + lateral 1x1`) and the GeM / MAC / SPoC pooling of layers/pooling.py:13-86, i.e. graph.minkfpn +
// graph.pool of egonn_amd/graph.py, on the kernels egonn_forward runs on.  egonn_minkfpn_finalize does once per model what the
// per-operator entry points do per call (BatchNorm folding, kernel packing); egonn_minkfpn_forward sizes every launch from the
// plan's capacities and the device row counts, so it runs on reserved plans without host synchronisation and can be captured.
#include "model.h"

using namespace egonn;

namespace egonn {

static constexpr int FPN_MAX_LEVELS = 7;

struct FpnBlock {
  BlockRef r;
  PackedKernel pk1, pk2;
};

struct MinkFpnModel {
  bool ready = false;
  int n_levels = 0, num_top_down = 0, feature_size = 0, block = 0, pooling = 0;
  int planes[FPN_MAX_LEVELS] = {}, layers[FPN_MAX_LEVELS] = {};
  const float* conv0 = nullptr;
  BnRef bn0;
  void* conv0_unit = nullptr;
  const float* convs[FPN_MAX_LEVELS] = {};
  BnRef bn[FPN_MAX_LEVELS];
  PackedKernel pk_convs[FPN_MAX_LEVELS];
  std::vector<FpnBlock> blocks[FPN_MAX_LEVELS];
  const float* c1x1[FPN_MAX_LEVELS + 1] = {};
  int c1x1_cin[FPN_MAX_LEVELS + 1] = {};
  const float* tconvs[FPN_MAX_LEVELS] = {};
  PackedKernel pk_t[FPN_MAX_LEVELS];
  const void* sp_t[FPN_MAX_LEVELS] = {};        // split packs of the top-down step (topdown.hip): tconv ndx, lateral ndx + 1
  const void* sp_l[FPN_MAX_LEVELS + 1] = {};
  const float* gem_p = nullptr;
  ModelStore store;
};

void minkfpn_model_free(MinkFpnModel* f) {
  if (!f) return;
  f->store.release();
  if (f->conv0_unit) (void)hipFree(f->conv0_unit);
  delete f;
}
void minkfpn_model_invalidate(MinkFpnModel* f) {
  if (f) f->ready = false;
}

}  // namespace egonn

namespace {

bool width_ok(int c) { return c == 32 || c == 64 || c == 128 || c == 256; }

// channels of the feature map of `level` (0 = the conv0 output)
int level_channels(const MinkFpnModel& f, int level) { return level == 0 ? f.planes[0] : f.planes[level - 1]; }

// shared argument check of finalize and out_level
int check_shape(const char* who, int n_levels, int num_top_down) {
  EGONN_REQUIRE(n_levels >= 1 && n_levels <= FPN_MAX_LEVELS, EGONN_ERR_INVALID, "%s: n_levels %d outside [1,%d]", who, n_levels, FPN_MAX_LEVELS);
  EGONN_REQUIRE(num_top_down >= 0 && num_top_down <= n_levels, EGONN_ERR_INVALID, "%s: num_top_down %d outside [0,%d] (n_levels)", who,
                num_top_down, n_levels);
  return EGONN_OK;
}

}  // namespace

API int egonn_minkfpn_out_level(int n_levels, int num_top_down, int* level) {
  EGONN_REQUIRE(level, EGONN_ERR_INVALID, "minkfpn_out_level: null out pointer");
  EGONN_TRY(check_shape("minkfpn_out_level", n_levels, num_top_down));
  *level = n_levels - num_top_down;
  return EGONN_OK;
}

API int egonn_minkfpn_finalize(egonn_model* m, int n_levels, const int* planes, const int* layers, int num_top_down, int feature_size,
                               int block, int pooling, void* stream) {
  EGONN_REQUIRE(m, EGONN_ERR_INVALID, "minkfpn_finalize: null model");
  EGONN_REQUIRE(planes && layers, EGONN_ERR_INVALID, "minkfpn_finalize: null planes / layers");
  EGONN_TRY(check_shape("minkfpn_finalize", n_levels, num_top_down));
  for (int i = 0; i < n_levels; ++i) {
    EGONN_REQUIRE(width_ok(planes[i]), EGONN_ERR_INVALID, "minkfpn_finalize: planes[%d] = %d (supported widths: 32, 64, 128, 256)", i, planes[i]);
    EGONN_REQUIRE(layers[i] >= 1 && layers[i] <= 64, EGONN_ERR_INVALID, "minkfpn_finalize: layers[%d] = %d outside [1,64]", i, layers[i]);
  }
  EGONN_REQUIRE(width_ok(feature_size), EGONN_ERR_INVALID, "minkfpn_finalize: feature_size %d (supported widths: 32, 64, 128, 256)", feature_size);
  EGONN_REQUIRE(planes[0] == 32, EGONN_ERR_INVALID,
                "minkfpn_finalize: planes[0] = %d: the k=5 one-channel input layer (conv0) is implemented for 32 output channels", planes[0]);
  EGONN_REQUIRE(block == 0 || block == 1, EGONN_ERR_INVALID, "minkfpn_finalize: block %d (0 = BasicBlock, 1 = ECABasicBlock)", block);
  EGONN_REQUIRE(pooling >= 0 && pooling <= 3, EGONN_ERR_INVALID, "minkfpn_finalize: pooling %d (0 = none, 1 = GeM, 2 = MAC, 3 = SPoC)", pooling);
  hipStream_t st = (hipStream_t)stream;
  if (!m->fpn) m->fpn = new MinkFpnModel();
  MinkFpnModel& f = *m->fpn;
  f.ready = false;
  f.n_levels = n_levels; f.num_top_down = num_top_down; f.feature_size = feature_size; f.block = block; f.pooling = pooling;
  const int L = n_levels, T = num_top_down, F = feature_size;
  for (int i = 0; i < L; ++i) { f.planes[i] = planes[i]; f.layers[i] = layers[i]; }

  // ---- resolve every tensor (shapes checked, the offending key named) and register what the store folds and packs: every
  // sparse-conv kernel once (fp32 fragments + split fragments where instantiated).  No device work before the last lookup.
  ModelStore& S = f.store;
  S.begin();
  EGONN_TRY(get_tensor(m, "backbone.conv0.kernel", {125, 1, planes[0]}, &f.conv0));
  EGONN_TRY(get_bn(m, "backbone.bn0", planes[0], &f.bn0, &S));
  for (int i = 0, inpl = planes[0]; i < L; ++i) {
    const std::string si = std::to_string(i);
    EGONN_TRY(get_tensor(m, "backbone.convs." + si + ".kernel", {8, inpl, inpl}, &f.convs[i]));
    EGONN_TRY(get_bn(m, "backbone.bn." + si, inpl, &f.bn[i], &S));
    S.add_kernel(f.convs[i], 8, inpl, inpl, false, &f.pk_convs[i]);
    f.blocks[i].assign((size_t)layers[i], FpnBlock());
    for (int j = 0, ci = inpl; j < layers[i]; ++j, ci = planes[i]) {
      FpnBlock& fb = f.blocks[i][j];
      EGONN_TRY(get_block(m, "backbone.blocks." + si + "." + std::to_string(j), ci, planes[i], block == 1, &fb.r, &S));
      S.add_kernel(fb.r.conv1, 27, ci, planes[i], false, &fb.pk1);
      S.add_kernel(fb.r.conv2, 27, planes[i], planes[i], false, &fb.pk2);
    }
    inpl = planes[i];
  }
  for (int i = 0; i <= T; ++i) {       // conv1x1[0]: the coarsest level; conv1x1[i]: the lateral of level L - i (models/minkfpn.py:47-58)
    f.c1x1_cin[i] = level_channels(f, L - i);
    EGONN_TRY(get_tensor(m, "backbone.conv1x1." + std::to_string(i) + ".kernel", {f.c1x1_cin[i], F}, &f.c1x1[i]));
  }
  for (int i = 0; i < T; ++i) {
    EGONN_TRY(get_tensor(m, "backbone.tconvs." + std::to_string(i) + ".kernel", {8, F, F}, &f.tconvs[i]));
    S.add_kernel(f.tconvs[i], 8, F, F, false, &f.pk_t[i]);
    f.sp_t[i] = f.sp_l[i + 1] = nullptr;
    if (topdown_split_supported(F, f.c1x1_cin[i + 1])) {      // the top-down step's own split packs
      S.add_pack(ModelStore::SPLIT, f.tconvs[i], 8, F, F, &f.sp_t[i]);
      S.add_pack(ModelStore::SPLIT, f.c1x1[i + 1], 1, f.c1x1_cin[i + 1], F, &f.sp_l[i + 1]);
    }
  }
  f.gem_p = nullptr;
  if (pooling == 1) {                  // MinkLoc wraps its pooling (layers/pooling.py:13-43), MinkLoc3D holds the GeM module itself
    const char* key = m->t.count("pooling.pooling.p") ? "pooling.pooling.p" : "pooling.p";
    EGONN_TRY(get_tensor(m, key, {1}, &f.gem_p));
  }

  // ---- device work from here on
  EGONN_TRY(S.commit(st));
  if (!f.conv0_unit) HIP_CHECK(hipMalloc(&f.conv0_unit, 2 * 4 * 3 * 64 * 16));
  EGONN_TRY(conv0_pack_unit(f.conv0, f.conv0_unit, st));
  f.ready = true;
  return EGONN_OK;
}

API int egonn_minkfpn_forward(egonn_ctx* c, egonn_model* m, int flags, float* out_global, float* out_map, void* stream) {
  EGONN_REQUIRE(out_global || out_map, EGONN_ERR_INVALID, "minkfpn_forward: out_global and out_map are both null");
  EGONN_REQUIRE((flags & ~EGONN_MINKFPN_SPLIT_TOPDOWN) == 0, EGONN_ERR_INVALID, "minkfpn_forward: unknown flags 0x%x", flags);
  EGONN_REQUIRE(m && m->fpn && m->fpn->ready, EGONN_ERR_INVALID, "minkfpn_forward: model not finalized (call egonn_minkfpn_finalize)");
  const MinkFpnModel& f = *m->fpn;
  EGONN_REQUIRE(f.pooling == 0 || out_global, EGONN_ERR_INVALID, "minkfpn_forward: out_global is null");
  EGONN_REQUIRE(f.pooling != 0 || out_map, EGONN_ERR_INVALID, "minkfpn_forward: out_map is null (a model without pooling returns the feature map)");
  EGONN_REQUIRE(c && c->plan.valid, EGONN_ERR_STATE, "no coordinate plan (call egonn_voxelize / egonn_coords_set first)");
  HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  Plan& P = c->plan;
  const int B = P.batch, L = f.n_levels, T = f.num_top_down, F = f.feature_size;
  const int32_t* cnt = c->dev_counts;                          // device row counts per level (the kernels clip to them)
  // the fp16 range flag covers THIS forward (see egonn_forward)
  HIP_CHECK(hipMemsetAsync(c->dev_fp16_flag, 0, sizeof(int32_t), st));

  // ---- row-group tables of every map the graph uses: one launch per plan
  {
    const int tlevels[FPN_MAX_LEVELS] = {0, 1, 2, 3, 4, 5, 6};      // the top-down steps' transposed maps: onto levels L - T .. L - 1
    EGONN_TRY(ensure_graph_rowgroups(c, L, tlevels + (L - T), T, st));
    DBG_SYNC("minkfpn row groups");
  }

  // ---- workspace: one layout sized from the capacities; every intermediate gets its own buffer
  size_t need = (size_t)P.cap[0] * f.planes[0] * 4 + 4096;
  for (int i = 0; i < L; ++i) {
    const size_t n = (size_t)P.cap[i + 1];
    need += n * 256 * 4 + 256;                                            // the strided convolution's output
    need += (size_t)f.layers[i] * (n * f.planes[i] * 4 * 4 + 4 * 256);   // per block: t1, t2, downsample branch, output
  }
  need += ((size_t)P.cap[L] + 64) * F * 4;
  for (int l = L - T; l < L; ++l) need += ((size_t)P.cap[l] + 64) * F * 4 * 2;
  need += ((size_t)B * SEG_CHUNKS * 256 + (size_t)B * 256 + 64) * 4 * 2 + (1u << 20);
  need += sconv_ksplit_scratch_floats(c) * 4 + 4096;
  Arena* A;
  EGONN_TRY(claim_work(c, need, true, &A));

  // per-scan scratch of the block tails and of the pooling: partial sums, the ECA gate right behind them (eca_apply)
  WALLOC(float, partial, (size_t)B * SEG_CHUNKS * 256 + (size_t)B * 256);

  // ---- conv0 on unit features (the reference always feeds ones): the occupancy-only first layer
  WALLOC(float, x0, P.cap[0] * f.planes[0]);
  {
    ProfScope ps(c, st, "conv0_k5_kernel/L0", PK_CONV0, 0, 125, 1, f.planes[0], 4);
    EGONN_TRY(conv0_k5_forward(c, nullptr, f.conv0, f.planes[0], f.bn0.scale, f.bn0.shift, 1, x0, 0, st, f.conv0_unit));
  }
  DBG_SYNC("minkfpn conv0");
  const float* feat[EGONN_NUM_LEVELS] = {x0};        // the map of every level (what the top-down pass reads as laterals)
  const float* x = x0;
  for (int i = 0; i < L; ++i) {
    const int lv = i + 1;
    const Level& V = P.lv[lv];
    const int64_t n = P.cap[lv];
    const int inpl = level_channels(f, i);
    WALLOC(float, y, n * inpl);
    EGONN_TRY(conv_layer(c, st, conv_call(1, lv, x, f.pk_convs[i], inpl, inpl, 0, &f.bn[i], 1, y), "k2s2"));
    DBG_SYNC("minkfpn L%d k2s2", lv);
    x = y;
    for (const FpnBlock& fb : f.blocks[i]) {       // graph.residual_block
      const BlockRef& b = fb.r;
      void* t2 = nullptr;
      EGONN_TRY(block_convs(c, st, A, lv, b, fb.pk1, fb.pk2, 0, x, nullptr, &t2));
      const float* res = x;
      if (b.down) {
        WALLOC(float, rd, n * b.cout);
        DenseCall dc = down_call(b, x, 0, n, cnt + lv, nullptr);
        dc.out = rd;
        EGONN_TRY(dense_forward(dc, st));
        res = rd;
      }
      WALLOC(float, xo, n * b.cout);
      EGONN_TRY(block_tail(static_cast<const float*>(t2), res, V.boff, B, n, b.cout, b.eca, b.eca_k, partial, xo, st));
      DBG_SYNC("minkfpn L%d block", lv);
      x = xo;
    }
    feat[lv] = x;
  }

  // ---- 1x1 of the coarsest level, then the top-down steps (graph.top_down): tconv + lateral 1x1
  const int out_level = L - T;
  float* g = nullptr;
  {
    float* dst = (T == 0 && out_map) ? out_map : nullptr;
    if (!dst) { WALLOC(float, gL, P.cap[L] * F); dst = gL; }
    EGONN_TRY(dense_forward({.in = feat[L], .n = P.cap[L], .n_dev = cnt + L, .cin = f.c1x1_cin[0], .cout = F, .W = f.c1x1[0], .out = dst}, st));
    g = dst;
  }
  const bool split_step = (flags & EGONN_MINKFPN_SPLIT_TOPDOWN) && sconv_split_arithmetic(c);
  for (int ndx = 0; ndx < T; ++ndx) {
    const int lo = L - 1 - ndx, cl = f.c1x1_cin[ndx + 1];
    float* dst = (lo == out_level && out_map) ? out_map : nullptr;
    if (!dst) { WALLOC(float, gx, P.cap[lo] * F); dst = gx; }
    if (split_step && f.sp_t[ndx]) {
      EGONN_TRY(topdown_split_forward(c, lo, g, f.sp_t[ndx], feat[lo], f.sp_l[ndx + 1], F, cl, dst, st));
    } else {
      WALLOC(float, u, P.cap[lo] * F);
      EGONN_TRY(conv_layer(c, st, conv_call(2, lo, g, f.pk_t[ndx], F, F, 0, nullptr, 0, u), "tconv"));
      // (the sum is commutative: bitwise `tconv + lateral`)
      EGONN_TRY(dense_forward({.in = feat[lo], .n = P.cap[lo], .n_dev = cnt + lo, .cin = cl, .cout = F, .W = f.c1x1[ndx + 1], .residual = u,
                               .out = dst},
                              st));
    }
    DBG_SYNC("minkfpn top-down onto L%d", lo);
    g = dst;
  }

  // ---- global pooling over the rows of the out level (layers/pooling.py:13-86)
  if (f.pooling != 0) {
    EGONN_TRY(global_pool((Pooling)f.pooling, g, P.lv[out_level].boff, B, F, f.gem_p, partial, out_global, st));
  }
  DBG_SYNC("minkfpn pooling");
  return EGONN_OK;
}

// One top-down step on its own (the operator egonn_minkfpn_forward uses; kernels in reference layout, packed per call)
API int egonn_topdown_step(egonn_ctx* c, int level_out, const float* x_coarse, const float* w_tconv, const float* x_lateral,
                           const float* w_lateral, int C, int Cl, float* out, void* stream) {
  EGONN_REQUIRE(level_out >= 0 && level_out < EGONN_NUM_LEVELS - 1, EGONN_ERR_INVALID, "topdown_step: level_out %d outside [0,6]", level_out);
  EGONN_REQUIRE(x_coarse && w_tconv && out, EGONN_ERR_INVALID, "topdown_step: null argument");
  EGONN_REQUIRE(!x_lateral || w_lateral, EGONN_ERR_INVALID, "topdown_step: x_lateral without w_lateral");
  EGONN_REQUIRE(topdown_split_supported(C, x_lateral ? Cl : 0), EGONN_ERR_INVALID,
                "topdown_step: channel plan C=%d, Cl=%d not supported (C 64/128/256, Cl a multiple of 32 up to C)", C, Cl);
  EGONN_REQUIRE((((uintptr_t)x_coarse | (uintptr_t)x_lateral | (uintptr_t)out) & 15) == 0, EGONN_ERR_INVALID,
                "topdown_step: feature maps must be 16-byte aligned");
  EGONN_REQUIRE(c && c->plan.valid, EGONN_ERR_STATE, "no coordinate plan (call egonn_voxelize / egonn_coords_set first)");
  HIP_CHECK(hipSetDevice(c->device));
  hipStream_t st = (hipStream_t)stream;
  Plan& P = c->plan;
  const size_t rows = (size_t)P.cap[level_out];
  const size_t sp_bytes = align_up(split_weights_bytes(8, C, C), 256) + align_up(split_weights_bytes(1, 256, C), 256);
  Arena* A;
  EGONN_TRY(claim_work(c, (SCONV_SCRATCH_FLOATS + sconv_ksplit_scratch_floats(c) + 2 * rows * C) * sizeof(float) + sp_bytes + 16384, true, &A));
  WALLOC(float, scratch, SCONV_SCRATCH_FLOATS);
  if (sconv_split_arithmetic(c)) {
    WALLOC(char, sp_t, align_up(split_weights_bytes(8, C, C), 256));
    WALLOC(char, sp_l, align_up(split_weights_bytes(1, 256, C), 256));
    EGONN_TRY(pack_split_weights(w_tconv, 8, C, C, 0, 0, sp_t, st));
    if (x_lateral) EGONN_TRY(pack_split_weights(w_lateral, 1, Cl, C, 0, 0, sp_l, st));
    return topdown_split_forward(c, level_out, x_coarse, sp_t, x_lateral, sp_l, C, Cl, out, st);
  }
  // exact fp32: the existing sequence — transposed convolution, 1x1, add (what egonn_conv_transpose / egonn_conv / egonn_add run)
  float* u = out;
  if (x_lateral) {
    WALLOC(float, ux, rows * C);
    u = ux;
  }
  const ConvCall cc{.kind = 2, .level = level_out, .in = x_coarse, .out = u, .cin = C, .cout = C, .W = w_tconv, .scratch = scratch,
                    .scratch_floats = SCONV_SCRATCH_FLOATS};
  EGONN_TRY(sconv_map(c, cc, st));
  if (!x_lateral) return EGONN_OK;
  WALLOC(float, v, rows * C);
  EGONN_TRY(dense_forward({.in = x_lateral, .n = P.lv[level_out].n, .cin = Cl, .cout = C, .W = w_lateral, .out = v}, st));
  return add_act(u, v, P.lv[level_out].n * C, 0, out, st);
}
