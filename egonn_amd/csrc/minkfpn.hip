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
  float* folded = nullptr;
  size_t folded_cap = 0;
  float* packed = nullptr;
  size_t packed_cap = 0;
};

void minkfpn_model_free(MinkFpnModel* f) {
  if (!f) return;
  if (f->folded) (void)hipFree(f->folded);
  if (f->packed) (void)hipFree(f->packed);
  if (f->conv0_unit) (void)hipFree(f->conv0_unit);
  delete f;
}
void minkfpn_model_invalidate(MinkFpnModel* f) {
  if (f) f->ready = false;
}

}  // namespace egonn

namespace {

bool width_ok(int c) { return c == 32 || c == 64 || c == 128 || c == 256; }

int eca_ksize(int c) {     // ECALayer kernel size (layers/eca_block.py:14-15): t = int(|log2(C) + 1| / 2), made odd
  int lg = 0;
  while ((1 << lg) < c) ++lg;
  const int t = (lg + 1) / 2;
  return (t % 2) ? t : t + 1;
}

// channels of the feature map of `level` (0 = the conv0 output)
int level_channels(const MinkFpnModel& f, int level) { return level == 0 ? f.planes[0] : f.planes[level - 1]; }

// shared argument check of finalize and out_level
int check_shape(const char* who, int n_levels, int num_top_down) {
  EGONN_REQUIRE(n_levels >= 1 && n_levels <= FPN_MAX_LEVELS, EGONN_ERR_INVALID, "%s: n_levels %d outside [1,%d]", who, n_levels, FPN_MAX_LEVELS);
  EGONN_REQUIRE(num_top_down >= 0 && num_top_down <= n_levels, EGONN_ERR_INVALID, "%s: num_top_down %d outside [0,%d] (n_levels)", who,
                num_top_down, n_levels);
  return EGONN_OK;
}

#define DBG_SYNC(...)                                                 \
  do {                                                                \
    if (switches().debug_sync) {                                      \
      fprintf(stderr, "[egonn] " __VA_ARGS__);                        \
      fprintf(stderr, "\n");                                          \
      fflush(stderr);                                                 \
      HIP_CHECK(hipStreamSynchronize(st));                            \
    }                                                                 \
  } while (0)

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

  // ---- resolve every tensor (shapes checked, the offending key named); count what the folded and packed stores must hold
  size_t n_bn = 1, need_p = 0, need_s = 0;        // BatchNorm layers; fp32 floats of the packed kernels; bytes of the split packs
  auto count_pack = [&](int K, int ci, int co) {
    need_p += (size_t)K * ci * co;
    if (sconv_split_supported(ci, co)) need_s += align_up(split_weights_bytes(K, ci, co), 256);
  };
  for (int i = 0, inpl = planes[0]; i < L; ++i) {
    n_bn += 1 + (size_t)layers[i] * 3;
    count_pack(8, inpl, inpl);
    for (int j = 0, ci = inpl; j < layers[i]; ++j, ci = planes[i]) { count_pack(27, ci, planes[i]); count_pack(27, planes[i], planes[i]); }
    inpl = planes[i];
  }
  for (int i = 0; i < T; ++i) {
    count_pack(8, F, F);
    need_s += align_up(split_weights_bytes(8, F, F), 256) + align_up(split_weights_bytes(1, 256, F), 256);   // the top-down step's own packs
  }
  // (the folded scale / shift slots are carved against a host stand-in and rebased once the device store exists: no device
  //  work before the last shape is checked)
  const size_t need_f = n_bn * 2 * 256;
  std::vector<float> stand_in(need_f);
  float* cur = stand_in.data();
  EGONN_TRY(get_tensor(m, "backbone.conv0.kernel", {125, 1, planes[0]}, &f.conv0));
  EGONN_TRY(get_bn(m, "backbone.bn0", planes[0], &f.bn0, &cur));
  for (int i = 0, inpl = planes[0]; i < L; ++i) {
    const std::string si = std::to_string(i);
    EGONN_TRY(get_tensor(m, "backbone.convs." + si + ".kernel", {8, inpl, inpl}, &f.convs[i]));
    EGONN_TRY(get_bn(m, "backbone.bn." + si, inpl, &f.bn[i], &cur));
    f.blocks[i].assign((size_t)layers[i], FpnBlock());
    for (int j = 0, ci = inpl; j < layers[i]; ++j, ci = planes[i]) {
      BlockRef& b = f.blocks[i][j].r;
      const int co = planes[i];
      b.cin = ci; b.cout = co;
      const std::string pre = "backbone.blocks." + si + "." + std::to_string(j);
      EGONN_TRY(get_tensor(m, pre + ".conv1.kernel", {27, ci, co}, &b.conv1));
      EGONN_TRY(get_bn(m, pre + ".norm1", co, &b.n1, &cur));
      EGONN_TRY(get_tensor(m, pre + ".conv2.kernel", {27, co, co}, &b.conv2));
      EGONN_TRY(get_bn(m, pre + ".norm2", co, &b.n2, &cur));
      b.down = nullptr;
      if (ci != co) {
        EGONN_TRY(get_tensor(m, pre + ".downsample.0.kernel", {ci, co}, &b.down));
        EGONN_TRY(get_bn(m, pre + ".downsample.1", co, &b.dn, &cur));
      }
      b.eca = nullptr; b.eca_k = 0;
      if (block == 1) {
        b.eca_k = eca_ksize(co);
        EGONN_TRY(get_tensor(m, pre + ".eca.conv.weight", {1, 1, b.eca_k}, &b.eca));
      }
    }
    inpl = planes[i];
  }
  for (int i = 0; i <= T; ++i) {       // conv1x1[0]: the coarsest level; conv1x1[i]: the lateral of level L - i (models/minkfpn.py:47-58)
    f.c1x1_cin[i] = level_channels(f, L - i);
    EGONN_TRY(get_tensor(m, "backbone.conv1x1." + std::to_string(i) + ".kernel", {f.c1x1_cin[i], F}, &f.c1x1[i]));
  }
  for (int i = 0; i < T; ++i) EGONN_TRY(get_tensor(m, "backbone.tconvs." + std::to_string(i) + ".kernel", {8, F, F}, &f.tconvs[i]));
  f.gem_p = nullptr;
  if (pooling == 1) {                  // MinkLoc wraps its pooling (layers/pooling.py:13-43), MinkLoc3D holds the GeM module itself
    const char* key = m->t.count("pooling.pooling.p") ? "pooling.pooling.p" : "pooling.p";
    EGONN_TRY(get_tensor(m, key, {1}, &f.gem_p));
  }

  // ---- device work from here on
  if (f.folded_cap < need_f) {
    if (f.folded) HIP_CHECK(hipFree(f.folded));
    f.folded = nullptr; f.folded_cap = 0;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&f.folded), need_f * sizeof(float)));
    f.folded_cap = need_f;
  }
  {
    auto rebase = [&](BnRef& r) {
      r.scale = f.folded + (r.scale - stand_in.data());
      r.shift = f.folded + (r.shift - stand_in.data());
    };
    rebase(f.bn0);
    for (int i = 0; i < L; ++i) {
      rebase(f.bn[i]);
      for (auto& b : f.blocks[i]) {
        rebase(b.r.n1);
        rebase(b.r.n2);
        if (b.r.down) rebase(b.r.dn);
      }
    }
  }
  // pack every sparse-conv kernel once (fp32 fragments + split fragments where instantiated)
  if (f.packed_cap < need_p * 4 + need_s + 1024) {
    if (f.packed) HIP_CHECK(hipFree(f.packed));
    f.packed = nullptr; f.packed_cap = 0;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&f.packed), need_p * 4 + need_s + 1024));
    f.packed_cap = need_p * 4 + need_s + 1024;
  }
  float* pc = f.packed;
  char* sc = reinterpret_cast<char*>(f.packed) + align_up(need_p * 4, 256);
  auto pack = [&](const float* w, int K, int ci, int co, PackedKernel* dst) -> int {
    EGONN_TRY(pack_rg_weights(w, K, ci, co, 0, 0, 0, pc, st));
    *dst = PackedKernel{pc, nullptr, nullptr};
    pc += (size_t)K * ci * co;
    if (sconv_split_supported(ci, co)) {
      EGONN_TRY(pack_split_weights(w, K, ci, co, 0, 0, sc, st));
      dst->split = sc;
      sc += align_up(split_weights_bytes(K, ci, co), 256);
    }
    return EGONN_OK;
  };
  auto pack_split_only = [&](const float* w, int K, int ci, int co, const void** dst) -> int {
    EGONN_TRY(pack_split_weights(w, K, ci, co, 0, 0, sc, st));
    *dst = sc;
    sc += align_up(split_weights_bytes(K, ci, co), 256);
    return EGONN_OK;
  };
  for (int i = 0, inpl = planes[0]; i < L; ++i) {
    EGONN_TRY(pack(f.convs[i], 8, inpl, inpl, &f.pk_convs[i]));
    for (auto& b : f.blocks[i]) {
      EGONN_TRY(pack(b.r.conv1, 27, b.r.cin, b.r.cout, &b.pk1));
      EGONN_TRY(pack(b.r.conv2, 27, b.r.cout, b.r.cout, &b.pk2));
    }
    inpl = planes[i];
  }
  for (int i = 0; i < T; ++i) {
    EGONN_TRY(pack(f.tconvs[i], 8, F, F, &f.pk_t[i]));
    f.sp_t[i] = f.sp_l[i + 1] = nullptr;
    if (topdown_split_supported(F, f.c1x1_cin[i + 1])) {
      EGONN_TRY(pack_split_only(f.tconvs[i], 8, F, F, &f.sp_t[i]));
      EGONN_TRY(pack_split_only(f.c1x1[i + 1], 1, f.c1x1_cin[i + 1], F, &f.sp_l[i + 1]));
    }
  }
  if (!f.conv0_unit) HIP_CHECK(hipMalloc(&f.conv0_unit, 2 * 4 * 3 * 64 * 16));
  EGONN_TRY(conv0_pack_unit(f.conv0, f.conv0_unit, st));
  // ---- fold every BatchNorm once
  EGONN_TRY(fold(f.bn0, st));
  for (int i = 0; i < L; ++i) {
    EGONN_TRY(fold(f.bn[i], st));
    for (auto& b : f.blocks[i]) {
      EGONN_TRY(fold(b.r.n1, st));
      EGONN_TRY(fold(b.r.n2, st));
      if (b.r.down) EGONN_TRY(fold(b.r.dn, st));
    }
  }
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
    int kinds[RG_MAX_JOBS], levels[RG_MAX_JOBS], nreq = 0;
    for (int l = 1; l <= L; ++l) { kinds[nreq] = 0; levels[nreq++] = l; }
    for (int l = 1; l <= L; ++l) { kinds[nreq] = 1; levels[nreq++] = l; }
    for (int l = L - T; l < L; ++l) { kinds[nreq] = 2; levels[nreq++] = l; }
    EGONN_TRY(ensure_rowgroups(c, kinds, levels, nreq, st));
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
  const size_t ks_floats = sconv_ksplit_scratch_floats(c);
  need += ks_floats * 4 + 4096;
  for (int l = 0; l < EGONN_NUM_LEVELS; ++l) c->level_feat[l] = nullptr;
  EGONN_TRY(c->work_arena.ensure(need));
  Arena& A = c->work_arena;
  A.reset();
  c->ks_part = ks_floats ? A.alloc<float>(ks_floats) : nullptr;
  c->ks_part_floats = c->ks_part ? ks_floats : 0;
#define WALLOC(var, count)                                                         \
  float* var = A.alloc<float>((size_t)(count));                                    \
  EGONN_REQUIRE(var != nullptr, EGONN_ERR_STATE, "work arena too small (" #var ")")

  // per-scan scratch of the block tails and of the pooling: partial sums, the ECA gate right behind them (eca_apply)
  WALLOC(partial, (size_t)B * SEG_CHUNKS * 256 + (size_t)B * 256);

  // ---- conv0 on unit features (the reference always feeds ones): the occupancy-only first layer
  WALLOC(x0, P.cap[0] * f.planes[0]);
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
    WALLOC(y, n * inpl);
    EGONN_TRY(conv_layer(c, st, conv_call(1, lv, x, f.pk_convs[i], inpl, inpl, 0, &f.bn[i], 1, y), "k2s2"));
    DBG_SYNC("minkfpn L%d k2s2", lv);
    x = y;
    for (const FpnBlock& fb : f.blocks[i]) {       // graph.residual_block
      const BlockRef& b = fb.r;
      WALLOC(t1, n * b.cout);
      // conv1's output has ONE reader, conv2: when both run on the split kernel it is written in split form (see egonn_forward)
      const bool t1_split = !switches().no_presplit && sconv_route(c, 0, lv, b.cin, b.cout, 0) == ROUTE_SPLIT &&
                            sconv_route(c, 0, lv, b.cout, b.cout, 0) == ROUTE_SPLIT;
      {
        ConvCall cc = conv_call(0, lv, x, fb.pk1, b.cin, b.cout, 0, &b.n1, 1, t1);
        cc.split_io = t1_split ? 2 : 0;
        EGONN_TRY(conv_layer(c, st, cc, "k3.conv1"));
      }
      WALLOC(t2, n * b.cout);
      {
        ConvCall cc = conv_call(0, lv, t1, fb.pk2, b.cout, b.cout, 0, &b.n2, 0, t2);
        cc.split_io = t1_split ? 1 : 0;
        EGONN_TRY(conv_layer(c, st, cc, "k3.conv2"));
      }
      const float* res = x;
      if (b.down) {
        WALLOC(rd, n * b.cout);
        EGONN_TRY(dense_forward({.in = x, .n = n, .n_dev = cnt + lv, .cin = b.cin, .cout = b.cout, .W = b.down, .scale = b.dn.scale,
                                 .shift = b.dn.shift, .out = rd},
                                st));
        res = rd;
      }
      WALLOC(xo, n * b.cout);
      if (b.eca) {                                   // ECABasicBlock tail: out = relu(t2 * sigmoid(conv1d(mean)) + res)
        EGONN_TRY(segment_partial_sums(t2, V.boff, B, b.cout, 0, nullptr, partial, st));
        EGONN_TRY(eca_apply(t2, res, partial, V.boff, B, n, b.cout, b.eca, b.eca_k, xo, st));
      } else {                                       // ME BasicBlock tail: out = relu(t2 + res)
        EGONN_TRY(add_act(t2, res, n * b.cout, 1, xo, st));
      }
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
    if (!dst) { WALLOC(gL, P.cap[L] * F); dst = gL; }
    EGONN_TRY(dense_forward({.in = feat[L], .n = P.cap[L], .n_dev = cnt + L, .cin = f.c1x1_cin[0], .cout = F, .W = f.c1x1[0], .out = dst}, st));
    g = dst;
  }
  const bool split_step = (flags & EGONN_MINKFPN_SPLIT_TOPDOWN) && sconv_split_arithmetic(c);
  for (int ndx = 0; ndx < T; ++ndx) {
    const int lo = L - 1 - ndx, cl = f.c1x1_cin[ndx + 1];
    float* dst = (lo == out_level && out_map) ? out_map : nullptr;
    if (!dst) { WALLOC(gx, P.cap[lo] * F); dst = gx; }
    if (split_step && f.sp_t[ndx]) {
      EGONN_TRY(topdown_split_forward(c, lo, g, f.sp_t[ndx], feat[lo], f.sp_l[ndx + 1], F, cl, dst, st));
    } else {
      WALLOC(u, P.cap[lo] * F);
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
    const int32_t* boff = P.lv[out_level].boff;
    if (f.pooling == 1) {
      EGONN_TRY(segment_partial_sums(g, boff, B, F, 1, f.gem_p, partial, st));
      EGONN_TRY(gem_finish(partial, boff, B, F, f.gem_p, out_global, st));
    } else {
      const int mode = f.pooling == 2 ? 2 : 0;
      EGONN_TRY(segment_partial_sums(g, boff, B, F, mode, nullptr, partial, st));
      EGONN_TRY(pool_finish(partial, boff, B, F, mode, out_global, st));
    }
  }
  DBG_SYNC("minkfpn pooling");
#undef WALLOC
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
  for (int l = 0; l < EGONN_NUM_LEVELS; ++l) c->level_feat[l] = nullptr;
  const size_t ks = sconv_ksplit_scratch_floats(c);
  const size_t rows = (size_t)P.cap[level_out];
  const size_t sp_bytes = align_up(split_weights_bytes(8, C, C), 256) + align_up(split_weights_bytes(1, 256, C), 256);
  c->ks_part = nullptr;
  c->ks_part_floats = 0;
  EGONN_TRY(c->work_arena.ensure((SCONV_SCRATCH_FLOATS + ks + 2 * rows * C) * sizeof(float) + sp_bytes + 16384));
  c->work_arena.reset();
  float* scratch = c->work_arena.alloc<float>(SCONV_SCRATCH_FLOATS);
  if (ks) {
    c->ks_part = c->work_arena.alloc<float>(ks);
    c->ks_part_floats = c->ks_part ? ks : 0;
  }
  if (sconv_split_arithmetic(c)) {
    char* sp_t = c->work_arena.alloc<char>(align_up(split_weights_bytes(8, C, C), 256));
    char* sp_l = c->work_arena.alloc<char>(align_up(split_weights_bytes(1, 256, C), 256));
    EGONN_REQUIRE(scratch && sp_t && sp_l, EGONN_ERR_STATE, "work arena too small");
    EGONN_TRY(pack_split_weights(w_tconv, 8, C, C, 0, 0, sp_t, st));
    if (x_lateral) EGONN_TRY(pack_split_weights(w_lateral, 1, Cl, C, 0, 0, sp_l, st));
    return topdown_split_forward(c, level_out, x_coarse, sp_t, x_lateral, sp_l, C, Cl, out, st);
  }
  // exact fp32: the existing sequence — transposed convolution, 1x1, add (what egonn_conv_transpose / egonn_conv / egonn_add run)
  float* u = x_lateral ? c->work_arena.alloc<float>(rows * C) : out;
  EGONN_REQUIRE(scratch && u, EGONN_ERR_STATE, "work arena too small");
  const ConvCall cc{.kind = 2, .level = level_out, .in = x_coarse, .out = u, .cin = C, .cout = C, .W = w_tconv, .scratch = scratch,
                    .scratch_floats = SCONV_SCRATCH_FLOATS};
  EGONN_TRY(sconv_map(c, cc, st));
  if (!x_lateral) return EGONN_OK;
  float* v = c->work_arena.alloc<float>(rows * C);
  EGONN_REQUIRE(v, EGONN_ERR_STATE, "work arena too small");
  EGONN_TRY(dense_forward({.in = x_lateral, .n = P.lv[level_out].n, .cin = Cl, .cout = C, .W = w_lateral, .out = v}, st));
  return add_act(u, v, P.lv[level_out].n * C, 0, out, st);
}
