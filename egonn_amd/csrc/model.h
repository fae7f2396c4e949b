// What the translation units behind the model entry points share (model.hip: EgoNN, minkfpn.hip: MinkLoc / MinkLoc3D): the
// context and model objects of the C ABI; the one way an entry point takes the context's work arena (claim_work + WALLOC); the
// state_dict lookups and the store both finalizers fill (ModelStore, get_block); and the pieces of a graph both models launch,
// each stated once: a sparse convolution, conv1 -> conv2 of a residual block, its downsample call, its un-fused tail, global
// pooling and the row-group request list.  Every file that defines an entry point includes it: the C header, the context behind
// egonn_ctx and its opening checks.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/egonn_hip.h"
#include "common.h"
#include "kernels.h"

struct egonn_ctx : public egonn::Ctx {
  // scratch kept between egonn_forward and its readers
  hipStream_t plan_stream = nullptr; // stream the current plan was enqueued on (lazy size queries synchronise it)

  void* level_feat[EGONN_NUM_LEVELS] = {};
  int level_ch[EGONN_NUM_LEVELS] = {};
  int level_bf16 = 0;                // precision of level_feat (last forward)
  bool from_points = false;
};

// the checks every entry point that reads the plan of a context starts with
#define REQUIRE_PLAN(c)                                                                               \
  EGONN_REQUIRE((c) && (c)->plan.valid, EGONN_ERR_STATE, "no coordinate plan (call egonn_voxelize / " \
                                                         "egonn_coords_set first)")
#define REQUIRE_LEVEL(c, level)                                                                              \
  REQUIRE_PLAN(c);                                                                                           \
  HIP_CHECK(hipSetDevice((c)->device));                                                                      \
  EGONN_REQUIRE((level) >= 0 && (level) < EGONN_NUM_LEVELS, EGONN_ERR_INVALID, "level %d out of range", (level))

// EGONN_DEBUG_SYNC=1: synchronise stream `st` after every stage of a forward and print its name (a GPU fault aborts the process
// at the next synchronisation: the last name printed is the stage that faulted).  Debug aid only; never set in captures.
#define DBG_SYNC(...)                                                 \
  do {                                                                \
    if (switches().debug_sync) {                                      \
      fprintf(stderr, "[egonn] " __VA_ARGS__);                        \
      fprintf(stderr, "\n");                                          \
      fflush(stderr);                                                 \
      HIP_CHECK(hipStreamSynchronize(st));                            \
    }                                                                 \
  } while (0)

// `count` elements of T from the claimed work arena `A` (an Arena* in scope), as `T* var`
#define WALLOC(T, var, count)                                                      \
  T* var = A->alloc<T>((size_t)(count));                                           \
  EGONN_REQUIRE(var != nullptr, EGONN_ERR_STATE, "work arena too small (" #var ")")

namespace egonn {

// The one way an entry point takes the context's work arena.  Whoever resets the arena retires everything that pointed into it:
// the level maps egonn_forward_level_features reads and the partial-tile scratch of the offset-split convolutions (ks_part).
// Grows the arena to `bytes` (synchronises the device when it grows), resets it and, with_ksplit, carves ks_part anew
// (sconv_ksplit_scratch_floats, which `bytes` must cover): every entry point that reaches sconv_map asks for it.
int claim_work(egonn_ctx* c, size_t bytes, bool with_ksplit, Arena** A);

struct TensorRef {
  const float* p = nullptr;
  std::vector<int64_t> shape;
};

struct BnRef {
  const float *w = nullptr, *b = nullptr, *rm = nullptr, *rv = nullptr;
  float *scale = nullptr, *shift = nullptr;
  int c = 0;
};

struct BlockRef {
  const float *conv1 = nullptr, *conv2 = nullptr, *down = nullptr, *eca = nullptr;
  BnRef n1, n2, dn;
  int cin = 0, cout = 0, eca_k = 0;
};

struct MlpRef {
  const float *w0 = nullptr, *b0 = nullptr, *w1 = nullptr, *b1 = nullptr;
  int cin = 0, mid = 0, cout = 0;
};

// The folded-BatchNorm buffer and the packed-kernel buffer of a model.  A finalizer registers what it resolves (nothing here
// touches the device), then commit() sizes both buffers from the registrations, allocates each once (growing only), and carves,
// packs and folds in registration order: no device call before the last state_dict lookup.
struct ModelStore {
  enum Form { RG32, RG16, SPLIT, DENSE, DENSE_OI };   // pack_rg_weights fp32 / bf16, pack_split_weights, dense_pack_frags of a
                                                       // (cin, cout) 1x1 kernel / of an (out, in) nn.Linear kernel
  struct Pack { Form form; const float* w; int K, ci, co; size_t off; const void** dst; };
  std::vector<BnRef*> bns;                  // the registered objects must stay where they are until commit()
  std::vector<Pack> packs;
  size_t bn_bytes = 0, pack_bytes = 0;      // every registration is 256-byte aligned
  char *folded = nullptr, *packed = nullptr;
  size_t folded_cap = 0, packed_cap = 0;

  void begin();
  void add_bn(BnRef* bn);
  void add_pack(Form form, const float* w, int K, int ci, int co, const void** dst);
  // a sparse-conv kernel W [K][ci][co]: the fp32 pack, the bf16 pack (models with a bf16 path), the split pack where
  // sconv_split_supported
  void add_kernel(const float* w, int K, int ci, int co, bool bf16, PackedKernel* dst);
  int commit(hipStream_t st);
  void release();
};

struct MinkFpnModel;                          // minkfpn.hip: the second model kind an egonn_model can be finalized as
void minkfpn_model_free(MinkFpnModel* f);
void minkfpn_model_invalidate(MinkFpnModel* f);

}  // namespace egonn

struct egonn_model {
  std::map<std::string, egonn::TensorRef> t;
  bool ready = false;
  egonn::ModelStore store;      // folded scale / shift of every BatchNorm; the sparse-conv kernels in MFMA fragment order
  // resolved views
  const float* conv0 = nullptr;
  egonn::BnRef bn[8];
  const float* convs[8] = {};
  egonn::BlockRef blk[8];
  const float *g1x1[8] = {}, *gt[8] = {}, *l1x1[8] = {}, *lt[8] = {};
  const float* gem_p = nullptr;
  egonn::MlpRef gdec, ldec, kp, sg;
  void* conv0_unit = nullptr;   // conv0_pack_unit(conv0): 24 KB
  void* lh_pack = nullptr;      // local_heads_pack: the heads' six Linear kernels as fp16 hi | lo fragments (92 KB)
  const float** lh_ptrs = nullptr;   // device array of the six weight pointers (the packer's input)
  egonn::PackedKernel pk_convs[8], pk_c1[8], pk_c2[8], pk_gt[8], pk_lt[8];   // fp32, bf16 (EGONN_FLAG_BF16) and fp16-split forms
  const void *pk_down[8] = {}, *pk_l1x1[8] = {};   // blk[i].down / l1x1[l] in the dense kernels' fragment order (dense_pack_frags; null: no such form)
  const void *pk_g1x1[8] = {}, *pk_gdec[2] = {};   // global_head.conv1x1[l] and the global decoder's two Linear kernels, the same order
  egonn::MinkFpnModel* fpn = nullptr;   // egonn_minkfpn_finalize: the MinkFPN view of the same tensors (minkfpn.hip)
};

namespace egonn {

// state_dict lookups: the tensor under `key` with exactly the shape `want`, else an error that names the key
int get_tensor(egonn_model* m, const std::string& key, std::initializer_list<int64_t> want, const float** out);
// the four tensors of `prefix`.bn.*; registers bn with the store (its scale / shift exist after commit)
int get_bn(egonn_model* m, const std::string& prefix, int c, BnRef* bn, ModelStore* store);
// the tensors of the residual block `prefix` (ECABasicBlock: eca), asked for in the order conv1, norm1, conv2, norm2,
// downsample.0, downsample.1 (ci != co), eca; its BatchNorms are registered
int get_block(egonn_model* m, const std::string& prefix, int ci, int co, bool eca, BlockRef* b, ModelStore* store);
int eca_ksize(int c);   // ECALayer kernel size (layers/eca_block.py:14-15): t = int(|log2(C) + 1| / 2), made odd
// One sparse convolution of a graph: the profiler tag "<kernel><cin,cout>/L<level>/<what>", the timing scope, the launch
int conv_layer(egonn_ctx* c, hipStream_t st, const ConvCall& cc, const char* what);
ConvCall conv_call(int kind, int level, const void* in, const PackedKernel& pk, int cin, int cout, int bf16, const BnRef* bn, int relu,
                   void* out);
// Row-group tables of the maps a graph uses, in ONE launch whose job order is the order here: k=3 of levels 1..L, k=2,s=2 of
// levels 1..L, then the transposed maps onto tlevels[0..nt)
int ensure_graph_rowgroups(egonn_ctx* c, int L, const int* tlevels, int nt, hipStream_t st);
// conv1 -> conv2 of a residual block on `level` (tags k3.conv1 / k3.conv2): *t2 = bn2(conv2(relu(bn1(conv1(in))))), both maps
// carved from A in the map precision.  conv1's output has ONE reader, conv2: when both run on the split kernel, conv1's epilogue
// writes it in split form (the fp16 hi | lo operands conv2 would otherwise make of every gathered fragment in its step loop;
// sconv_split.hip).  psum (nullable): [row groups][cout] column sums of t2
int block_convs(egonn_ctx* c, hipStream_t st, Arena* A, int level, const BlockRef& b, const PackedKernel& pk1, const PackedKernel& pk2,
                int bf16, const void* in, float* psum, void** t2);
// the 1x1 downsample branch of a block with its BatchNorm on the n rows of `in`; the caller sets `out` and what rides on it
DenseCall down_call(const BlockRef& b, const void* in, int bf16, int64_t n, const int32_t* n_dev, const void* wfrag);
// the un-fused tail of a block on n rows of fp32 maps: out = relu(x * sigmoid(conv1d(mean)) + res) (eca: ECABasicBlock) or
// relu(x + res) (ME BasicBlock).  partial: B * SEG_CHUNKS * ch + B * ch floats
int block_tail(const float* x, const float* res, const int32_t* boff, int B, int64_t n, int ch, const float* eca, int eca_k,
               float* partial, float* out, hipStream_t st);
// global pooling of a row map (layers/pooling.py:13-86): the codes of egonn_minkfpn_finalize's `pooling`
enum Pooling { POOL_GEM = 1, POOL_MAC = 2, POOL_SPOC = 3 };
int global_pool(Pooling method, const float* x, const int32_t* boff, int B, int C, const float* p, float* partial, float* out,
                hipStream_t st);   // p: the GeM exponent (device); partial: B * SEG_CHUNKS * C floats
// The tail of the global head on the fp32 rows of g5 (capacity ncap, live count n_dev, scans boff): out[b] = pooling of
// decoder(g5 rows of scan b).  fused: one launch leaves the pooling's partial sums (global_tail_fused; needs global_tail_fusable
// and the decoder's packed kernels pk[0..1]); else the decoder's two dense launches write gh (ncap x mid) and gd (ncap x cout) and
// the partial sums are a third.  Bitwise the same `partial` and `out` either way.
bool global_tail_fusable(const MlpRef& r);
int global_tail(const MlpRef& r, const void* const* pk, const float* g5, int64_t ncap, const int32_t* n_dev, const int32_t* boff, int B,
                Pooling method, const float* p, bool fused, float* gh, float* gd, float* partial, float* out, hipStream_t st);

// topdown.hip: one top-down step of an FPN on the fp16-split pipe,
//   out[o] = x_coarse[parent(o)] @ W_t[key(o) & 7] (+ x_lateral[o] @ W_l)
// sp_tconv / sp_lateral: pack_split_weights of the (8, C, C) and (1, Cl, C) kernels.  Rows come from the transposed map's row-group
// tables onto `level_out` (ensure_rowgroups kind 2); the epilogue raises SPLIT_RANGE_BIT of the plan's fp16 flag word on a non-finite accumulator.
bool topdown_split_supported(int C, int Cl);
int topdown_split_forward(Ctx* ctx, int level_out, const float* x_coarse, const void* sp_tconv, const float* x_lateral,
                          const void* sp_lateral, int C, int Cl, float* out, hipStream_t stream);

}  // namespace egonn
