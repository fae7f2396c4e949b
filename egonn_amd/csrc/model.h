// What the translation units behind the model entry points share (model.hip: EgoNN, minkfpn.hip: MinkLoc / MinkLoc3D): the
// context and model objects of the C ABI, the state_dict lookups and the one way a graph launches a sparse convolution.
// Every file that defines an entry point includes it: the C header, the context behind egonn_ctx and its opening checks.
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

namespace egonn {

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

struct MinkFpnModel;                          // minkfpn.hip: the second model kind an egonn_model can be finalized as
void minkfpn_model_free(MinkFpnModel* f);
void minkfpn_model_invalidate(MinkFpnModel* f);

}  // namespace egonn

struct egonn_model {
  std::map<std::string, egonn::TensorRef> t;
  bool ready = false;
  float* folded = nullptr;      // scale/shift storage
  size_t folded_cap = 0;
  // resolved views
  const float* conv0 = nullptr;
  egonn::BnRef bn[8];
  const float* convs[8] = {};
  egonn::BlockRef blk[8];
  const float *g1x1[8] = {}, *gt[8] = {}, *l1x1[8] = {}, *lt[8] = {};
  const float* gem_p = nullptr;
  egonn::MlpRef gdec, ldec, kp, sg;
  // sparse-conv kernels repacked into MFMA fragment order (one buffer, carved in finalize)
  float* packed = nullptr;
  size_t packed_cap = 0;
  void* conv0_unit = nullptr;   // conv0_pack_unit(conv0): 24 KB
  void* lh_pack = nullptr;      // local_heads_pack: the heads' six Linear kernels as fp16 hi | lo fragments (92 KB)
  const float** lh_ptrs = nullptr;   // device array of the six weight pointers (the packer's input)
  egonn::PackedKernel pk_convs[8], pk_c1[8], pk_c2[8], pk_gt[8], pk_lt[8];   // fp32, bf16 (EGONN_FLAG_BF16) and fp16-split forms
  const float *pk_down[8] = {}, *pk_l1x1[8] = {};   // blk[i].down / l1x1[l] in the dense kernels' fragment order (dense_pack_frags), in `packed`
  egonn::MinkFpnModel* fpn = nullptr;   // egonn_minkfpn_finalize: the MinkFPN view of the same tensors (minkfpn.hip)
};

namespace egonn {

// state_dict lookups: the tensor under `key` with exactly the shape `want`, else an error that names the key
int get_tensor(egonn_model* m, const std::string& key, std::initializer_list<int64_t> want, const float** out);
// the four tensors of `prefix`.bn.* and room for the folded scale / shift at *cursor (advanced by 2 c floats)
int get_bn(egonn_model* m, const std::string& prefix, int c, BnRef* bn, float** cursor);
int fold(const BnRef& bn, hipStream_t st);
// One sparse convolution of a graph: the profiler tag "<kernel><cin,cout>/L<level>/<what>", the timing scope, the launch
int conv_layer(egonn_ctx* c, hipStream_t st, const ConvCall& cc, const char* what);
ConvCall conv_call(int kind, int level, const void* in, const PackedKernel& pk, int cin, int cout, int bf16, const BnRef* bn, int relu,
                   void* out);

// topdown.hip: one top-down step of an FPN on the fp16-split pipe,
//   out[o] = x_coarse[parent(o)] @ W_t[key(o) & 7] (+ x_lateral[o] @ W_l)
// sp_tconv / sp_lateral: pack_split_weights of the (8, C, C) and (1, Cl, C) kernels.  Rows come from the transposed map's row-group
// tables onto `level_out` (ensure_rowgroups kind 2); the epilogue raises bit 3 of `flags` on a non-finite accumulator.
bool topdown_split_supported(int C, int Cl);
int topdown_split_forward(Ctx* ctx, int level_out, const float* x_coarse, const void* sp_tconv, const float* x_lateral,
                          const void* sp_lateral, int C, int Cl, float* out, hipStream_t stream);

}  // namespace egonn
