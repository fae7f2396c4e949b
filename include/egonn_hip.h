/* libegonn_hip — C ABI of the MI355X-native EgoNN descriptor-extraction path.
 *
 * Drop-in boundary: the reference (jac99/Egonn) has no native code; its
 * hot path crosses into the third-party MinkowskiEngine 0.5.4 Python bindings.  Each entry point below
 * cites the reference call site (file:line under /root/reference) whose MinkowskiEngine call it
 * replaces.  All pointers are raw device pointers (unless marked HOST), all sizes are explicit, there
 * are no torch types in any signature.  Every call enqueues its work on `stream` (a hipStream_t passed
 * as void*); the only host synchronisations are the size queries marked [SYNC].
 *
 * Conventions
 *   - return value: 0 = ok, non-zero = error; egonn_last_error() returns a thread-local message.
 *   - coordinates: int32 [batch, x, y, z] rows, exactly ME's `batched_coordinates` layout.
 *   - rows of every level are stored in Z-order of (batch, x, y, z): batch-contiguous, deterministic.
 *     (ME's own row order is hash-iteration order and unspecified; consumers may only rely on the
 *     coordinate <-> row association, which egonn_level_coords exposes.)
 *   - levels: level l has tensor stride 2^l (coordinates are multiples of 2^l), l = 0..7.
 *   - fp32 everywhere; sparse-conv kernels are (K, Cin, Cout) / (Cin, Cout), Linear weights (out, in):
 *     the reference's own state_dict layouts.
 */
#ifndef EGONN_HIP_H
#define EGONN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct egonn_ctx egonn_ctx;       /* one per (device, stream user); owns the coordinate plan + workspace */
typedef struct egonn_model egonn_model;   /* EgoNN weights registered by state_dict key */

enum { EGONN_QUANT_CARTESIAN = 0, EGONN_QUANT_POLAR = 1 };
/* status codes returned by every entry point (0 = ok; egonn_last_error() holds the text) */
enum { EGONN_STATUS_OK = 0, EGONN_STATUS_INVALID = 1, EGONN_STATUS_HIP = 2, EGONN_STATUS_RANGE = 3, EGONN_STATUS_STATE = 4,
       EGONN_STATUS_CAPACITY = 5,
       /* an fp32 sparse convolution on the fp16-split matrix pipe met a non-finite accumulator (an activation beyond +-65504,
        * or a non-finite input): the batch's outputs are invalid; egonn_ctx_set_exact_fp32(ctx, 1) and run it again */
       EGONN_STATUS_FP16_RANGE = 6 };
enum { EGONN_FLAG_DISABLE_GLOBAL = 1, EGONN_FLAG_DISABLE_LOCAL = 2, EGONN_FLAG_IGNORE_KP_REGRESSOR = 4,
       /* BASELINE configs[2]: feature maps and sparse-conv weights are bf16 in HBM (2 bytes per element), products
        * accumulate in fp32 on v_mfma_f32_16x16x32_bf16; the dense heads, pooling and all outputs stay fp32 */
       EGONN_FLAG_BF16 = 8,
       /* global pooling of PoolingWrapper (layers/pooling.py:13-43) other than the default GeM: SPoC = average, MAC = max */
       EGONN_FLAG_POOL_SPOC = 16, EGONN_FLAG_POOL_MAC = 32 };

/* ------------------------------------------------------------------ lifecycle / errors */
/* coord_bits in [10,16]: voxel coordinates must lie in [-2^(coord_bits-1), 2^(coord_bits-1)). */
int egonn_ctx_create(egonn_ctx** ctx, int device, int coord_bits);
void egonn_ctx_destroy(egonn_ctx* ctx);
const char* egonn_last_error(void);
/* tests / measurements only: which kernel this context's sparse convolutions run on.  Never set by the product path.  The codes:
 *     0   the product choice (so is every other code below 1000 that is not listed here)
 *     1   the plain one-thread-per-output HIP kernel, every layer: the cross-check of the MFMA kernels
 *     2   the register-ring per-tile kernel (exact fp32 / bf16)
 *     4   the workgroup-cooperative kernel
 *     8   the register-ring kernel with two groups per wave
 *    16   the LDS-DMA kernel, split-phase LDS fetch, 4 ring slots (fp32 maps; bf16 maps: the register-ring kernel)
 *    32   the LDS-DMA kernel with the fetch inside the item, 3 ring slots
 *   128   the traced build of the LDS-DMA kernel (egonn_debug_set_trace; 32->32 and 64->64, other plans untraced)
 *   1000 + cfg   the fp16-split kernel on every fp32 map it is instantiated for, in the configuration cfg; cfg 0 = its default
 *                (142, or EGONN_SPLIT_CFG).  cfg = shape [+ 400 * (1 + log2(column parts per task))] [+ 9000: the traced build],
 *                shape = 100 + 10 * NW + 2: lock-step workgroups of NW = 4 or 8 waves (142, 182), or 183: the weight-resident
 *                form (32->32 only).  Without the 400s term the layer's own rule picks the column parts.  A cfg whose shape has
 *                no instantiation is an error of the convolution, not of this call.
 * Codes 2 .. 128 compute bitwise the same results; the exact kernels and the split kernel differ by the split's rounding. */
int egonn_debug_set_naive_conv(egonn_ctx* ctx, int on);
/* tests / measurements only: the offset-split rule of this context's fp32 sparse convolutions on the small maps (the rule is
 * a function of (map class, output level), never of the batch).  map_class 0 = the k=3 maps, 1 = the 8-slot maps (k=2,s=2 and
 * transposed); kparts = offset parts as separate workgroups + a fixed-order reducer launch (1 = none); kw = offset parts inside a
 * workgroup (0 / 1 = none, 2..4); col_parts = column parts per task (0 = automatic); -1 keeps a field.  Every setting sums a
 * row's offsets in a fixed partition and order: results are deterministic and batch-invariant under each, and differ between
 * settings by summation order only (<= 3e-6 of the largest output; tests/test_gpu_ksplit.py). */
int egonn_debug_set_ksplit(egonn_ctx* ctx, int map_class, int level, int kparts, int kw, int col_parts);
/* tests / measurements only: which 32->32 fp16-split convolutions of this context run on the weight-resident form of the split
 * kernel (the whole packed kernel staged into LDS once per workgroup, no barrier in the offset loop).  mask bit 0 = the k=3
 * convolutions of level 1, bit 1 = the k=2,s=2 convolution into level 1, bit 2 = the gated k=2,s=2 convolution into level 2;
 * -1 = the product rule.  max_workgroups: workgroups per resident launch, 0 = default (also applies to the explicit
 * configuration egonn_debug_set_naive_conv(ctx, 1183)).  Every setting computes bitwise the same results
 * (tests/test_gpu_resident_conv.py). */
int egonn_debug_set_resident(egonn_ctx* ctx, int mask, int max_workgroups);
/* tests only: on = 1 makes egonn_forward materialise the block output of every level, so that egonn_forward_level_features(ctx, 1, ...)
 * has a map to return (by default level 1's block tail of fp32 maps is evaluated inside level 2's strided convolution and its
 * 23 MB output never exists; bitwise the same results either way) */
int egonn_debug_keep_level_features(egonn_ctx* ctx, int on);
/* measurement hook: buffer for the traced sparse-conv builds (code 128, cfg 9000 + shape): 8 u64 per wave task; NULL = off */
int egonn_debug_set_trace(void* device_buffer);
/* measurement hook: device copies of a map's row-group tables (gmask [groups], snbr [groups][K][16], nullable).  [SYNC] */
int egonn_debug_rowgroup_tables(egonn_ctx* ctx, int map_kind, int level_out, uint32_t* gmask_out, int32_t* snbr_out,
                                int64_t capacity_groups, int64_t* n_groups, void* stream);
/* test hook: device copy of the same map's perm table ([groups][16] int32: the output row of every slot, -1 = padding); with
 * the two tables above it is the whole row-group form.  Never called by the product path.  [SYNC] */
int egonn_debug_rowgroup_perm(egonn_ctx* ctx, int map_kind, int level_out, int32_t* perm_out, int64_t capacity_groups,
                              int64_t* n_groups, void* stream);
/* test hook: the two radix sorts of egonn_amd/csrc/sort.hip on their own, with every argument their call sites use.  Never
 * called by the product path; needs no context: the sort's histograms live in a borrowed span of the caller's scratch.
 * seg_offsets NULL: the flat sort of the first n pairs (n_dev nullable: DEVICE int64 count, clipped to n; n_segments =
 * idx_bits = 0).  either_pair = 0: the result is in (keys_out, vals_out); 1: in whichever pair the last pass wrote.
 * seg_offsets given (DEVICE int64, n_segments + 1, clipped to n): every segment [seg_offsets[b], seg_offsets[b+1]) is sorted
 * on its own, rows outside the segments are not touched; idx_bits = 0: (key, value) pairs; idx_bits > 0: keys_in holds packed
 * elements (sort bits << idx_bits | index inside the segment; vals_in is not read) and the result is key = (segment << nbits) |
 * (packed >> idx_bits), value = clipped seg_offsets[segment] + index.  n_dev must be NULL, either_pair is ignored.
 * Both sorts are stable and carry keys whole.  They read WHOLE DIGITS above the first sorted bit (bit 0, or idx_bits): 8 bits
 * per pass and ceil(nbits / 8) passes flat, 9 bits per pass and ceil(nbits / 9) passes (8 at most) segmented, so key bits
 * between nbits and the end of the last digit take part in the order; bits from there on are carried and never read.
 * result_pair (HOST): 0 = the result is in (keys_in, vals_in), 1 = in (keys_out, vals_out); the other pair is clobbered
 * below the count.  scratch: egonn_debug_radix_sort_scratch_bytes(n, n_segments) bytes (n_segments = 0: the flat sort;
 * -1 on bad arguments), 256-byte aligned.  No host synchronisation. */
int64_t egonn_debug_radix_sort_scratch_bytes(int64_t n, int n_segments);
int egonn_debug_radix_sort(uint64_t* keys_in, uint32_t* vals_in, uint64_t* keys_out, uint32_t* vals_out, int64_t n, int nbits,
                           const int64_t* n_dev, const int64_t* seg_offsets, int n_segments, int idx_bits, int either_pair,
                           int32_t* result_pair, void* scratch, int64_t scratch_bytes, void* stream);
/* test hook: the tail of the global head (descriptor decoder Linear 128 -> 192 + ReLU, Linear 192 -> 256, then the global
 * pooling) on the caller's rows, without a context or a model.  g5: DEVICE fp32 (rows_capacity, 128); row_offsets: DEVICE int32
 * (batch_size + 1), the rows of scan b are [row_offsets[b], row_offsets[b+1]), all below the live count n_dev (DEVICE int32,
 * <= rows_capacity); rows from the live count on are never read.  w0 (192, 128), b0, w1 (256, 192), b1: the decoder in nn.Linear
 * layout; pooling: 1 = GeM with the exponent p (DEVICE), 2 = MAC, 3 = SPoC (p nullable).  form 0: the decoder as two dense
 * launches, then the partial sums; form 1: one fused launch on the kernels in fragment order.  partial: DEVICE
 * (batch_size, 32 chunks, 256) partial sums of the pooling; out: DEVICE (batch_size, 256).  Both forms give the same bits.
 * scratch: egonn_debug_global_tail_scratch_bytes(rows_capacity) bytes (-1 on a bad capacity), 256-byte aligned.  No host
 * synchronisation. */
/* test hook: the grouped lateral launch of MinkHead — three independent (n_q, 128) @ (128, 128) products, fp32 rows, (cin, cout)
 * kernels, no epilogue — on the caller's DEVICE buffers.  The arrays are HOST arrays of three entries: in[q] (rows_capacity[q], 128),
 * n_dev[q] (DEVICE int32 live count <= rows_capacity[q]; rows from it on are not written), weight[q], out[q]; packed[q] = the
 * kernel in fragment order (egonn_dense_pack_fragments) for all three, or NULL for all three: the raw kernels are gathered.  Every
 * capacity must be one the dense launcher gives its small kernel (below 8192 rows).  Both forms give the bits of egonn_dense. */
int egonn_debug_dense_group3(const float* const in[3], const int64_t rows_capacity[3], const int32_t* const n_dev[3],
                             const float* const weight[3], const float* const packed[3], float* const out[3], void* stream);
int64_t egonn_debug_global_tail_scratch_bytes(int64_t rows_capacity);
int egonn_debug_global_tail(const float* g5, const int32_t* row_offsets, int batch_size, int64_t rows_capacity, const int32_t* n_dev,
                            const float* w0, const float* b0, const float* w1, const float* b1, const float* p, int pooling, int form,
                            float* partial, float* out, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ coordinate plan
 * replaces ME.utils.sparse_quantize      datasets/quantization.py:42,83   (Cartesian/Polar quantizer __call__)
 *          ME.utils.batched_coordinates  eval/evaluate.py:333, datasets/dataset_utils.py:77
 *          ME.SparseTensor(...)          models/minkgl.py:269             (coordinate-map build)
 *          ME coordinate manager         strided maps + kernel maps of every conv in models/minkgl.py:100-134,39-43
 */
/* Voxelise B scans.  points: (n,3) f32 device, scan b = rows [scan_offsets[b], scan_offsets[b+1]) (HOST, B+1
 * entries).  step: HOST, 1 value (Cartesian) or 3 (polar: degrees, metres, metres).  Builds the plan for the
 * voxelised batch.  [SYNC] */
int egonn_voxelize(egonn_ctx* ctx, const float* points, const int64_t* scan_offsets, int batch_size, int quant_mode,
                   const float* step, void* stream);
/* Capturable plans.  egonn_ctx_reserve fixes the sizes of everything a plan allocates: at most max_points input rows,
 * exactly batch_size scans, at most level_capacity[l] voxels at level l = 0..7 (HOST, 8 entries; NULL = max_points for every
 * level).  After it, egonn_voxelize_device builds the plan WITHOUT any host synchronisation or allocation: points (n_rows,3)
 * f32 device with n_rows <= max_points (rows beyond scan_offsets_dev[B] are ignored), scan_offsets_dev DEVICE int64 (B+1).
 * The per-level row counts stay in device memory, every kernel of egonn_forward / egonn_select_keypoints clips to them,
 * so the sequence voxelize_device -> forward -> select_keypoints can be captured into a hipGraph once and replayed on
 * other batches.  Outputs of a reserved plan are sized by the capacities (out_descriptors: level_capacity[3] rows).
 * egonn_plan_status [SYNC] copies the sizes and the error state of the latest (replayed) plan to the host: non-zero if a
 * coordinate left the +-2^(coord_bits-1) range (status 3) or the batch did not fit the reservation (status 5 =
 * EGONN_STATUS_CAPACITY; the outputs are then invalid — checking the status is MANDATORY for reserved plans: out-of-range /
 * non-finite points are clamped into their sample and overflowing rows are clipped, so an unchecked batch yields
 * plausible-looking but wrong descriptors); afterwards egonn_level_count / egonn_level_batch_offsets return that batch's true sizes.
 * What a status read covers: the coordinate / capacity state of the latest plan, and the fp16 range flag (status 6, see
 * egonn_ctx_set_exact_fp32) of everything run on the plan since the start of the latest egonn_forward — every forward clears that
 * flag in stream order (captured with it), so a forward on the same plan after egonn_ctx_set_exact_fp32(ctx, 1) reports only
 * itself; operator calls (egonn_sparse_conv, training steps) add to it until the next forward or plan. */
int egonn_ctx_reserve(egonn_ctx* ctx, int64_t max_points, int batch_size, const int64_t* level_capacity);
int egonn_voxelize_device(egonn_ctx* ctx, const float* points, int64_t n_rows, const int64_t* scan_offsets_dev,
                          int batch_size, int quant_mode, const float* step, void* stream);
int egonn_plan_status(egonn_ctx* ctx, void* stream);
/* Arithmetic of the fp32 sparse convolutions of this context (models/minkgl.py:105 -> ME's fp32 GEMM).  on = 0 (default): the
 * maps of levels <= 5 run on the fp16 matrix pipe with split operands — x = hi + lo with fp16 parts (|x - hi - lo| <= 2^-22 |x|),
 * weights scaled by a power of two per kernel, the three products hi*hi + hi*lo + lo*hi on v_mfma_f32_16x16x32_f16 with fp32
 * accumulation: within 3e-6 of the plain fp32 kernel relative to the largest output (tests/test_gpu_graph.py,
 * tests/test_gpu_ksplit.py), the low part of an activation below 2^-3 carrying an ABSOLUTE error <= 2^-25.  The two claims meet
 * at small operands: the 3e-6 relative bound holds for maps whose largest |entry| is at least 2^-4.5 (measured: it stops holding
 * between 2^-4.6 and 2^-5.0 on four layer shapes, tests/test_gpu_range_edges.py); below that only the absolute bound holds, per
 * output |err| <= 2^-25 * sum over the gathered offsets and input channels of |W| (plus fp32 rounding) — scale such operands up
 * (egonn_ctx_set_operand_autoscale) or use on = 1.  RANGE: an fp16 part holds |x| < 65520 (65504 <= |x| < 65520 round to 65504
 * with an exact low part); an activation at or beyond that, or a non-finite one, turns every accumulator that gathers it into
 * Inf / NaN, which the kernels' epilogues detect before BatchNorm / ReLU can hide it, and the local heads test their input
 * before splitting it: egonn_plan_status (eager and reserved plans alike) then returns EGONN_STATUS_FP16_RANGE for that batch —
 * there is no silent overflow.  on = 1: every level on the exact fp32 kernels (v_mfma_f32_16x16x4_f32: fp32's range, 1/16 of the
 * matrix rate) and the exact heads.  The 128 -> 128 maps of levels 6-7 run the same split arithmetic on the per-tile kernel,
 * guarded the same way; bf16 maps and channel plans without a split instantiation always run the exact kernels (the local heads
 * of bf16 maps are split and guarded). */
int egonn_ctx_set_exact_fp32(egonn_ctx* ctx, int on);
/* on = 1: the fp16-split convolutions of this context scale their INPUT map by a power of two per launch (max |in| -> [2^13, 2^14),
 * one reduction launch, undone exactly in the epilogue) — for operands far below 1: the input-gradient convolutions of a training
 * step (training/trainer.py:160-175 -> loss.backward()), whose entries of 1e-6 .. 1e-8 would otherwise lose their fp16 low parts.
 * Eager plans only: refused with EGONN_ERR_STATE on a reserved context (the scale reads the map's row count on the host), and
 * egonn_ctx_reserve refuses a context that has it on.  Default 0 (activations of a forward pass sit well inside the range). */
int egonn_ctx_set_operand_autoscale(egonn_ctx* ctx, int on);
/* Row capacity of a level of the current plan (= its row count for eager plans).  No sync. */
int egonn_level_capacity(egonn_ctx* ctx, int level, int64_t* capacity);
/* hipGraph capture of a sequence of calls on `stream` (hipStreamBeginCapture / EndCapture + Instantiate / hipGraphLaunch):
 * for hosts without their own HIP binding.  Everything between begin and end must be capturable: a reserved context that
 * has run the same sequence once (so that no arena grows), no [SYNC] entry point. */
typedef struct egonn_graph egonn_graph;
int egonn_graph_begin(void* stream);
int egonn_graph_end(void* stream, egonn_graph** graph);
int egonn_graph_launch(egonn_graph* graph, void* stream);
void egonn_graph_destroy(egonn_graph* graph);
/* Build the plan from explicit coordinates (N,4) int32 [b,x,y,z] in any row order; duplicate rows collapse onto
 * their first occurrence (ME SparseTensor default).  [SYNC] */
int egonn_coords_set(egonn_ctx* ctx, const int32_t* coords, int64_t n, int batch_size, void* stream);

/* Queries on the current plan (HOST results, no sync: filled by the size query of the call above). */
int egonn_level_count(egonn_ctx* ctx, int level, int64_t* n_rows);
int egonn_level_batch_offsets(egonn_ctx* ctx, int level, int64_t* offsets /* HOST, B+1 */);
/* (N_l,4) int32 coordinates of level `level` in row order. */
int egonn_level_coords(egonn_ctx* ctx, int level, int32_t* out, void* stream);
/* For level-0 row i: index of the caller's point / coordinate row it came from (first occurrence).
 * For egonn_voxelize the index is relative to the scan's own first point, as the reference quantizer returns. */
int egonn_input_index(egonn_ctx* ctx, int64_t* out /* (N0,) device */, void* stream);

/* ------------------------------------------------------------------ operators on the current plan
 * (per-operator entry points; egonn_forward below chains them on device)                                  */
/* MinkowskiConvolution: kernel_size 5 (level_out==level_in==0, Cin=1), 3 (same level), 2 (stride 2,
 * level_out = level_in+1), 1 (dense).  models/minkgl.py:100,105,43,124; ME BasicBlock conv1/conv2.
 * scale/shift (nullable): folded eval-mode MinkowskiBatchNorm; relu: fused MinkowskiReLU. */
int egonn_conv(egonn_ctx* ctx, int level_in, int level_out, int kernel_size, const float* in, int cin,
               const float* kernel, int cout, const float* scale, const float* shift, int relu, float* out,
               void* stream);
/* MinkowskiConvolutionTranspose(k=2,s=2) onto the cached finer map: models/minkgl.py:39,53. level_out = level_in-1 */
int egonn_conv_transpose(egonn_ctx* ctx, int level_in, const float* in, int cin, const float* kernel, int cout,
                         float* out, void* stream);
/* The operator behind the two calls above, with explicit map and precision.  map_kind 0: kernel_size 3 on level_out;
 * 1: kernel_size 2 / stride 2 from level_out-1 into level_out; 2: transposed (k=2,s=2) from level_out+1 onto level_out.
 * bf16 = 1: `in` and `out` are bf16 feature maps (BASELINE configs[2]); the fp32 kernel is rounded to bf16, products
 * accumulate in fp32.  group_sums (nullable): (n_groups, cout) fp32 column sums of the output per group of 16 rows
 * (egonn_map_groups) — the conv2 epilogue form of MinkowskiGlobalPooling (layers/eca_block.py:16,26).  With bf16 maps the
 * sums are taken over the fp32 values BEFORE they are rounded to bf16 for storage (the pooled mean is then the mean of the
 * unrounded activations: closer to the fp32 path than a mean of the stored bf16 numbers; within the configs[2] tolerance).
 * fp32 maps of levels <= 5, and the 128 -> 128 maps of levels 6-7, run on the fp16 matrix pipe with split operands (fp16 hi +
 * lo parts, three products, fp32 accumulate, range guard and small-operand limit: see egonn_ctx_set_exact_fp32 above; deviation
 * from the exact fp32 kernel < 3e-6 of the largest output); the maps of levels 3-5 sum a row's offsets in a fixed partition (egonn_debug_set_ksplit).  Non-finite inputs: Inf
 * comes out as NaN / Inf and raises the range flag; NaN stays NaN on both paths. */
int egonn_sparse_conv(egonn_ctx* ctx, int map_kind, int level_out, const void* in, int cin, const float* kernel, int cout,
                      int bf16, const float* scale, const float* shift, int relu, void* out, float* group_sums,
                      void* stream);
/* Builds the row-group tables of every kernel map of the current plan in one launch (otherwise each operator builds the tables
 * of its map on first use): k=3 and k=2,s=2 maps of levels 1..7, transposed maps onto levels 1..6 and, with
 * with_level0_transpose, onto level 0 (input gradient of the first strided convolution, training/trainer.py:168).  No sync. */
int egonn_prepare_maps(egonn_ctx* ctx, int with_level0_transpose, void* stream);
/* n_groups / first_group (HOST, B+1 entries, nullable) of a map's row groups.  [SYNC] */
int egonn_map_groups(egonn_ctx* ctx, int map_kind, int level_out, int64_t* n_groups, int64_t* first_group, void* stream);
/* MinkowskiGlobalAvgPooling: layers/eca_block.py:16, layers/pooling.py:80.  out (B,C) */
int egonn_global_avg_pool(egonn_ctx* ctx, int level, const float* in, int channels, float* out, void* stream);

/* MinkowskiBatchNorm in eval mode (= nn.BatchNorm1d on the rows) folded to per-channel scale/shift for the fused
 * epilogue of egonn_conv:  scale = weight / sqrt(running_var + eps),  shift = bias - running_mean * scale. */
int egonn_bn_fold(const float* weight, const float* bias, const float* running_mean, const float* running_var,
                  float eps, int channels, float* scale, float* shift, void* stream);
/* Tail of a residual block: out = relu(x * gate + residual).  eca_weight (k,) non-NULL: ECALayer gate
 * (MinkowskiGlobalPooling -> Conv1d over channels -> sigmoid -> MinkowskiBroadcastMultiplication,
 * layers/eca_block.py:21-36,66-71); NULL: plain ME BasicBlock tail (out += residual; relu). */
int egonn_block_tail(egonn_ctx* ctx, int level, const float* x, const float* residual, int channels,
                     const float* eca_weight, int eca_ksize, float* out, void* stream);
/* SparseTensor + SparseTensor on the same coordinate map (models/minkfpn.py:91, models/minkgl.py:56). */
int egonn_add(const float* a, const float* b, int64_t n, float* out, void* stream);
/* batch['features'] (caller row order of egonn_coords_set) -> plan row order, (N0, channels). */
int egonn_gather_input(egonn_ctx* ctx, const float* features, int channels, float* out, void* stream);
/* GeM pooling (layers/pooling.py:82-86, third_party/minkloc3d/minkloc.py:47-59): out (B, channels). */
int egonn_gem(egonn_ctx* ctx, int level, const float* x, int channels, const float* p, float* out, void* stream);
/* MAC pooling, MinkowskiGlobalMaxPooling (layers/pooling.py:46-56): out (B, channels), per-sample column max (0 for an
 * empty sample).  channels <= 256 and a divisor of 256. */
int egonn_global_max_pool(egonn_ctx* ctx, int level, const float* in, int channels, float* out, void* stream);
/* NetVLAD / NetVLAD-GC pooling of MinkLoc in eval mode: NetVLADWrapper (layers/pooling.py:89-109) around NetVLADLoupe
 * (layers/netvlad.py:18-80, cluster_size 64, add_batch_norm=True) and GatingContext (layers/netvlad.py:83-112).
 * x (N_l, channels) rows of level `level` in plan row order; out (B, out_dim).  Weights are raw device pointers in the
 * reference layout: cluster_weights (C, 64), cluster_weights2 (1, C, 64), hidden1_weights (C*64, out_dim), gating_weights
 * (out_dim, out_dim); bn1 / bn2 / gate scale+shift are the eval-mode BatchNorms folded by egonn_bn_fold (64 / out_dim /
 * out_dim entries).  gating 0 = 'netvlad' (gating pointers ignored, may be NULL), 1 = 'netvladgc'.
 * Pad rule: the reference zero-pads every scan to Nmax = max_b n_b rows (pad_sequence, layers/pooling.py:103); each pad row
 * adds softmax(bn1 shift) to the cluster mass a_sum, so a scan's descriptor depends on Nmax of its batch.  That term is
 * reproduced, with Nmax taken from the plan's device-side row offsets.
 * Limits: channels % 16 == 0 and 16 <= channels <= 512; out_dim % 16 == 0 and 16 <= out_dim <= 1024; clusters fixed at 64;
 * x 16-byte aligned.  Anything else returns EGONN_STATUS_INVALID.  Exact fp32 (f32 MFMA / FMA), four launches, no host
 * sync, workspace from the context: capturable on one stream; bitwise reproducible and independent of the other scans'
 * order in the batch. */
int egonn_netvlad(egonn_ctx* ctx, int level, const float* x, int channels, const float* cluster_weights,
                  const float* cluster_weights2, const float* bn1_scale, const float* bn1_shift,
                  const float* hidden1_weights, const float* bn2_scale, const float* bn2_shift,
                  const float* gating_weights, const float* gate_scale, const float* gate_shift, int out_dim, int gating,
                  float* out, void* stream);
/* NetVLAD / NetVLAD-GC in TRAIN mode, the part of NetVLADLoupe.forward (layers/netvlad.py:44-73, under NetVLADWrapper's
 * pad_sequence, layers/pooling.py:97-109) that works on rows: out (B, out_dim) = normalize(normalize_c(V)) @ hidden1_weights,
 * BEFORE bn2 (bn2 and the context gating are (B, out_dim) row operators: egonn_col_stats / egonn_bn_train_finalize /
 * egonn_affine_act, egonn_dense, egonn_sigmoid_gate).  Layouts and limits as egonn_netvlad; B >= 2 (batch statistics).
 * bn1 / pad rule: bn1 normalises the logits Z = X @ cluster_weights of all M = B * nmax rows of the zero-padded batch, nmax =
 * the largest scan of the level (HOST value, from egonn_level_batch_offsets).  A pad row has Z = 0, so mean = (sum_real z) / M
 * and the biased variance (sum_real z^2) / M - mean^2, formed in fp64 around bn1_running_mean; every pad row then has the logits
 * beta - mean * gamma * invstd, the folded shift, and adds softmax(shift) to the cluster mass exactly as in eval mode.  The
 * running statistics are updated in place (momentum, unbiased factor M / (M - 1)); num_batches_tracked is the caller's.
 * Saved for the backward (caller-owned): save_z (N_l, 64) = Z, save_bn1 (4, 64) = mean, invstd, scale, shift, save_v
 * (B, channels, 64) = V before the normalisations, save_sq (B, channels / 16, 64) its squared-norm partials, save_asum (B, 64).
 * Exact fp32 (f32 MFMA / FMA), fp64 BatchNorm sums, no atomics, no host synchronisation, workspace from the context. */
int egonn_netvlad_train_forward(egonn_ctx* ctx, int level, const float* x, int channels, int nmax,
                                const float* cluster_weights, const float* cluster_weights2, const float* bn1_weight,
                                const float* bn1_bias, float bn1_eps, float bn1_momentum, float* bn1_running_mean,
                                float* bn1_running_var, const float* hidden1_weights, int out_dim, float* out, float* save_z,
                                float* save_bn1, float* save_v, float* save_sq, float* save_asum, void* stream);
/* Its backward: grad_out (B, out_dim) -> grad_x (N_l, channels), grad_cluster_weights (channels, 64), grad_cluster_weights2
 * (channels, 64), grad_hidden1_weights (channels * 64, out_dim) and out_bn1 (5, 64) whose rows 3 and 4 are the gradients of
 * bn1's weight and bias (rows 0-2: the coefficients of dZ = a dL + b Z + c).  The (nmax - n_b) pad rows of every scan are
 * added analytically to bn1's sums (assignment softmax(shift), dA = da_sum_b, z - mean = -mean): they carry gradient into
 * gamma, beta, the mean and the variance.  The two F.normalize backwards keep the reference's eps 1e-12 clamps.
 * Summation orders: rows in chunks that are a function of the scan's own row count (128-row target, at most 32), chunks in
 * order, scans in batch order; bitwise reproducible; a scan's rows of grad_x depend on the other scans only through the
 * bn1 vectors and nmax.  Same limits, same arithmetic and workspace rules as the forward. */
int egonn_netvlad_train_backward(egonn_ctx* ctx, int level, const float* x, int channels, int nmax,
                                 const float* cluster_weights, const float* cluster_weights2, const float* bn1_weight,
                                 const float* hidden1_weights, int out_dim, const float* grad_out, const float* save_z,
                                 const float* save_bn1, const float* save_v, const float* save_sq, const float* save_asum,
                                 float* grad_x, float* grad_cluster_weights, float* grad_cluster_weights2, float* out_bn1,
                                 float* grad_hidden1_weights, void* stream);
/* MAC pooling with its argmax: out (B, channels) as egonn_global_max_pool, out_rows (B, channels) int32 = the plan row that
 * holds the maximum (-1 for an empty sample).  Tie rule: the LOWEST plan row wins.  [ME-recall, unpinned]: which of two tied
 * rows MinkowskiGlobalMaxPooling routes the gradient to is not checked against MinkowskiEngine (absent from the build); the
 * fixtures hold no tie.  Any channels >= 1. */
int egonn_global_max_pool_argmax(egonn_ctx* ctx, int level, const float* in, int channels, float* out, int32_t* out_rows,
                                 void* stream);
/* Its backward: grad_in (N_l, channels) = 0 except grad_in[rows[b][c]][c] = grad_out[b][c]; an empty sample gets nothing. */
int egonn_global_max_pool_backward(egonn_ctx* ctx, int level, const float* grad_out, const int32_t* rows, int channels,
                                   float* grad_in, void* stream);
/* GatingContext's product (layers/netvlad.py:108-110) on n values: grad_out NULL: out = y * sigmoid(t); else
 * grad_y = grad_out * s and grad_t = grad_out * y * s * (1 - s), s = sigmoid(t). */
int egonn_sigmoid_gate(const float* y, const float* t, const float* grad_out, int64_t n, float* out, float* grad_y,
                       float* grad_t, void* stream);

/* ------------------------------------------------------------------ model
 * replaces model_factory(...) / MinkGL.forward: models/model_factory.py:31-76, models/minkgl.py:267-315       */
int egonn_model_create(egonn_model** model);
void egonn_model_destroy(egonn_model* model);
/* Register a tensor by its reference state_dict key.  The pointer is borrowed and must
 * stay valid until it is re-registered or the model is destroyed. */
int egonn_model_set_tensor(egonn_model* model, const char* key, const float* data, int ndim, const int64_t* shape);
/* Validate keys/shapes, fold eval-mode BatchNorm into scale/shift.  Call again whenever weights change. */
int egonn_model_finalize(egonn_model* model, void* stream);

/* Forward on the current plan.  features: for an egonn_coords_set plan (n_input, 1) f32 in the CALLER's row
 * order (batch['features'], eval/evaluate.py:334); for an egonn_voxelize plan (N0, 1) in level-0 row order
 * (the voxels did not exist before the call, so there is no caller order).  features == NULL means "all ones" (what
 * the reference always feeds, eval/evaluate.py:334) and selects the occupancy-only first layer.  Outputs (caller-allocated, sizes from egonn_level_count):
 *   out_global (B,256) ; out_descriptors (N3,128) unit-L2 ; out_keypoints (N3,3) metres ; out_sigma (N3,1)
 * rows in level-3 row order (per-sample splits = egonn_level_batch_offsets(3)).  Any output may be NULL when
 * the corresponding head is disabled through `flags`.  quant_mode/step as in egonn_voxelize (needed for
 * Quantizer.keypoint_position, datasets/quantization.py:60-72,93-103).  No host sync. */
int egonn_forward(egonn_ctx* ctx, egonn_model* model, const float* features, int quant_mode, const float* step,
                  int flags, float* out_global, float* out_descriptors, float* out_keypoints, float* out_sigma,
                  void* stream);
/* Feature map of a trunk level produced by the last egonn_forward (debug / parity tests): (N_l, C_l).  Levels whose block output
 * egonn_forward does not materialise return EGONN_ERR_STATE: with fp32 maps level 1's block output is evaluated on the fly by the
 * strided convolution into level 2 (EGONN_NO_GATED_K2S2=1 in the environment materialises it again). */
int egonn_forward_level_features(egonn_ctx* ctx, int level, float* out, int channels, void* stream);

/* ------------------------------------------------------------------ MinkLoc / MinkLoc3D: MinkFPN + pooling in one call
 * replaces MinkFPN.forward (models/minkfpn.py:65-93) + PoolingWrapper.forward (layers/pooling.py:13-43) in eval mode.
 *
 * The second kind an egonn_model can be finalized as.  The tensors are registered with egonn_model_set_tensor under the
 * reference's state_dict keys: backbone.conv0.kernel, backbone.bn0.bn.*, backbone.convs.i.kernel, backbone.bn.i.bn.*,
 * backbone.blocks.i.j.{conv1,norm1,conv2,norm2,downsample.0,downsample.1,eca.conv}, backbone.conv1x1.i.kernel,
 * backbone.tconvs.i.kernel and, for GeM, pooling.pooling.p (MinkLoc) or pooling.p (MinkLoc3D).  Checks every shape (the error
 * names the key), folds every BatchNorm and packs every sparse-conv kernel ONCE.  Supported: n_levels 1..7; planes[i] and
 * feature_size in {32, 64, 128, 256} with planes[0] = 32 (the k=5 one-channel input layer); layers[i] >= 1;
 * num_top_down 0..n_levels; block 0 = BasicBlock, 1 = ECABasicBlock; pooling 0 = none (feature map only), 1 = GeM, 2 = MAC,
 * 3 = SPoC.  Anything else returns EGONN_STATUS_INVALID before any device work.  Call again whenever weights change. */
int egonn_minkfpn_finalize(egonn_model* model, int n_levels, const int* planes, const int* layers, int num_top_down,
                           int feature_size, int block, int pooling, void* stream);
/* Level of the feature map the top-down pass ends on (n_levels - num_top_down): out_map of the forward below holds
 * egonn_level_capacity of that level rows. */
int egonn_minkfpn_out_level(int n_levels, int num_top_down, int* level);
/* The whole eval graph on the current plan (eager or reserved) as one fixed launch sequence; unit input features (what the
 * reference always feeds).  out_global (B, feature_size): the pooled descriptor (required unless pooling = 0); out_map
 * (nullable; capacity of the out level x feature_size): the feature map the pooling reads, rows in plan order (only the rows
 * in use are written).  flags: EGONN_MINKFPN_SPLIT_TOPDOWN runs every top-down step as ONE launch on the fp16 matrix pipe
 * (egonn_topdown_step's split arithmetic; ignored on an exact-fp32 context); 0 keeps the exact sequence transposed
 * convolution + 1x1 + add.  Clears the fp16 range flag at its start like egonn_forward; no allocation after the first
 * call on a plan size, no host synchronisation: capturable on a reserved context.  The result of a scan does not depend on
 * the capacities, on the other scans of the batch or on eager versus replayed execution. */
enum { EGONN_MINKFPN_SPLIT_TOPDOWN = 1 };
int egonn_minkfpn_forward(egonn_ctx* ctx, egonn_model* model, int flags, float* out_global, float* out_map, void* stream);
/* One top-down step of a feature pyramid (models/minkfpn.py:86-91) onto level_out, rows in plan order:
 *   out[o] = x_coarse[parent(o)] @ w_tconv[key(o) & 7]  (+ x_lateral[o] @ w_lateral)
 * x_coarse (N_{level_out+1}, C), w_tconv (8, C, C), x_lateral (N_level_out, Cl) nullable, w_lateral (Cl, C), out (N_level_out, C);
 * C in {64, 128, 256}, Cl a multiple of 32 up to C; feature maps 16-byte aligned.  Default context: both products on
 * v_mfma_f32_16x16x32_f16 with split operands (fp16 hi + lo, three products, fp32 accumulate): |out - exact| <=
 * 3e-6 max |out|; a non-finite accumulator (an operand beyond the fp16 range) raises EGONN_STATUS_FP16_RANGE in
 * egonn_plan_status.  After egonn_ctx_set_exact_fp32(ctx, 1): bitwise egonn_conv_transpose, the 1x1 egonn_conv and
 * egonn_add in that order. */
int egonn_topdown_step(egonn_ctx* ctx, int level_out, const float* x_coarse, const float* w_tconv, const float* x_lateral,
                       const float* w_lateral, int C, int Cl, float* out, void* stream);

/* Keypoint selection — MinkLocGLEvaluator.get_keypoints_idxes, eval/evaluate.py:352-361: per sample the n_k
 * keypoints with the lowest sigma in increasing order (ties: Z-order of the super-voxel).  Padded outputs:
 *   sel_keypoints (B,n_k,3), sel_descriptors (B,n_k,128), sel_rows (B,n_k) level-3 row or -1, sel_count (B,). */
int egonn_select_keypoints(egonn_ctx* ctx, const float* sigma, const float* keypoints, const float* descriptors,
                           int n_k, float* sel_keypoints, float* sel_descriptors, int32_t* sel_rows,
                           int32_t* sel_count, void* stream);

/* The selection alone on explicit segments: row_offsets DEVICE int32 (batch_size+1), sel_rows (batch_size,n_k) global row or
 * -1, sel_count (batch_size,). */
int egonn_topk_rows(const float* sigma, const int32_t* row_offsets, int batch_size, int n_k, int32_t* sel_rows,
                    int32_t* sel_count, void* stream);

/* ------------------------------------------------------------------ batch-hard triplet loss (training, configs[3])
 * replaces BatchHardTripletLossWithMasks.__call__ (models/loss.py:146-172; miner :114-143; the distance / loss /
 * reducer it calls are pytorch_metric_learning's LpDistance(p=2), TripletMarginLoss(swap=True), AvgNonZeroReducer).
 * embeddings (n,d) f32 — in the sharded step the RCCL all-gathered matrix; masks (n,n) u8.
 * out_stats (10 f32, device): loss, num_triplets, num_non_zero_triplets, avg_embedding_norm, mean/max/min hardest
 * positive distance, mean/max/min hardest negative distance.  out_triplets (n,3) i32: anchor (or -1 if dropped),
 * hardest positive, hardest negative.  out_grad (n,d) nullable: dLoss/dEmbeddings.  scratch: device floats,
 * egonn_triplet_loss_scratch_floats(n) of them.  No host sync. */
int64_t egonn_triplet_loss_scratch_floats(int n);
int egonn_triplet_loss(const float* embeddings, int n, int d, const uint8_t* positives_mask,
                       const uint8_t* negatives_mask, float margin, float* out_stats, int32_t* out_triplets,
                       float* out_grad, float* scratch, void* stream);

/* ------------------------------------------------------------------ batch-hard contrastive loss (training)
 * replaces BatchHardContrastiveLossWithMasks.__call__ (models/loss.py:175-204; selected by `loss = BatchHardContrastiveLoss`,
 * models/loss.py:17-18, margins misc/utils.py:158-160) on the same distances and the same miner as egonn_triplet_loss
 * (models/loss.py:114-143).  The loss it calls is pytorch_metric_learning's ContrastiveLoss(pos_margin, neg_margin,
 * LpDistance(p=2, power=1), AvgNonZeroReducer), restated from its documentation [recall]: the mined triplets are read as the
 * pairs (a,p) and (a,n); pos_i = relu(D[a][p] - pos_margin), neg_i = relu(neg_margin - D[a][n]) on the plain (not squared)
 * Euclidean distance; each set is averaged over its entries > 0 (0 if none) and the two means are added.  No swap.
 * out_stats (13 f32, device): loss, num_triplets, pos_pairs_above_threshold, neg_pairs_above_threshold, pos_loss, neg_loss,
 * avg_embedding_norm, mean/max/min hardest positive distance, mean/max/min hardest negative distance.  out_triplets,
 * out_grad (nullable; a zero distance contributes no gradient) and scratch (egonn_contrastive_loss_scratch_floats(n) device
 * floats) as in egonn_triplet_loss.  No host sync. */
int64_t egonn_contrastive_loss_scratch_floats(int n);
int egonn_contrastive_loss(const float* embeddings, int n, int d, const uint8_t* positives_mask,
                           const uint8_t* negatives_mask, float pos_margin, float neg_margin, float* out_stats,
                           int32_t* out_triplets, float* out_grad, float* scratch, void* stream);

/* ------------------------------------------------------------------ local-head losses (training)
 * replaces the dense torch.cdist / torch.min / CrossEntropyLoss work of KeypointLoss (models/loss_utils.py:23-95) and
 * CorrespondenceLoss (:108-139), driven per pair of scans by KeypointCorrLoss (models/loss.py:43-92).  The kernels return
 * indices, distances and d loss / d logits; the differentiable tail on (n,3)/(n,1) tensors is the host's autograd. */
/* Nearest row of b (m,3) for every row of a (n,3), a optionally transformed first by the row-major 4x4 `transform`
 * (misc/poses.py:68-76; device pointer, NULL = none): torch.min(torch.cdist(a', b), dim=1) without the matrix. */
int egonn_nn_search(const float* a, int64_t n, const float* transform, const float* b, int64_t m, float* out_dist,
                    int32_t* out_index, void* stream);
/* torch.min(d, dim=1) and torch.min(d, dim=0) of a dense (n,m) matrix: values and indices (ties: lowest index). */
int egonn_matrix_min(const float* d, int64_t n, int64_t m, float* row_min, int32_t* row_index, float* col_min,
                     int32_t* col_index, void* stream);
/* nn.CrossEntropyLoss rows on (n,m) logits: target (n) int32, < 0 = row ignored.  out_loss (n), out_argmax (n),
 * out_dlogits (n,m) = softmax - onehot (nullable). */
int egonn_softmax_cross_entropy(const float* logits, int64_t n, int64_t m, const int32_t* target, float* out_loss,
                                int32_t* out_argmax, float* out_dlogits, void* stream);

/* The whole KeypointCorrLoss (models/loss.py:32-92) of a batch of (anchor, positive) pairs in ONE call: the second half of the
 * training step (training/trainer.py:186-190).  Loss, every metric and d out_batch[0] / d input for the six keypoint, sigma and
 * descriptor arrays, with the arithmetic of the per-pair driver (egonn_amd/local_loss.py): searches on exact differences (ties:
 * lowest index), probabilistic chamfer + point-to-point terms (a zero distance has a zero gradient), row-wise softmax
 * cross-entropy over exp(beta) * desc1 . desc2^T on the rows whose nearest kp2 lies within dist_th, in exact fp32 FMAs.  No
 * (n1 x n2) matrix is stored: the logits are evaluated tile by tile in LDS.  No host sync, no float atomics: two calls agree
 * bitwise, and a pair's row of out_pair does not depend on its position in the batch.
 * Argument order differs from a plain list of arrays in one way: the totals come first, BY VALUE (they size the launches).
 *   pairs >= 1; n_cloud1/2, n_kp1/2 >= 1: rows of the packed arrays; dim: descriptor width, 128 only.
 *   clouds (M,3), kp (N,3), sigma (N), desc (N,dim; 16-byte aligned), *_off (pairs+1) int32 DEVICE offsets of every pair's rows
 *   (every pair needs at least one keypoint on both sides and one point in both clouds), transforms (pairs,16) DEVICE row-major
 *   4x4 taking scan 1 into scan 2's frame, params HOST 6 floats: gamma_chamfer, gamma_p2p, gamma_c, gamma_k, beta, dist_th.
 *   out_pair (pairs, EGONN_LOCAL_LOSS_STATS), out_batch (EGONN_LOCAL_LOSS_STATS) = mean over the pairs; columns
 *   EGONN_LL_*.  A pair without a keypoint within dist_th has a NaN correspondence_loss and loss (CrossEntropyLoss over no
 *   rows), so the batch loss is NaN, and NaN descriptor gradients — and nothing else of it is NaN.
 *   g_*: same shapes as the inputs, all six or none (NULL = loss and metrics only).
 *   scratch: egonn_local_loss_scratch_bytes(pairs, n_kp1, n_kp2, dim) DEVICE bytes, 256-byte aligned. */
#define EGONN_LOCAL_LOSS_STATS 16
enum { EGONN_LL_LOSS = 0, EGONN_LL_KP_PER_CLOUD = 1, EGONN_LL_REPEATABILITY = 2, EGONN_LL_CHAMFER_PURE = 3,
       EGONN_LL_CHAMFER_WEIGHTED = 4, EGONN_LL_MEAN_SIGMA = 5, EGONN_LL_LOSS_CHAMFER = 6, EGONN_LL_LOSS_P2P = 7,
       EGONN_LL_KEYPOINT_LOSS = 8, EGONN_LL_CORRESPONDENCE_LOSS = 9, EGONN_LL_MATCHING_KEYPOINTS = 10,
       EGONN_LL_MATCHING_DESCRIPTORS = 11, EGONN_LL_POS_SIMILARITY = 12, EGONN_LL_NEG_SIMILARITY = 13 /* 14, 15: zero */ };
int64_t egonn_local_loss_scratch_bytes(int pairs, int64_t n_kp1, int64_t n_kp2, int dim);
int egonn_local_loss(int pairs, int64_t n_cloud1, int64_t n_cloud2, int64_t n_kp1, int64_t n_kp2, int dim,
                     const float* clouds1, const int32_t* cloud_off1, const float* clouds2, const int32_t* cloud_off2,
                     const float* kp1, const float* sigma1, const float* desc1, const int32_t* kp_off1,
                     const float* kp2, const float* sigma2, const float* desc2, const int32_t* kp_off2,
                     const float* transforms, const float* params, float* out_pair, float* out_batch,
                     float* g_kp1, float* g_sigma1, float* g_desc1, float* g_kp2, float* g_sigma2, float* g_desc2,
                     void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ training-mode operators (configs[3])
 * The reference trains through MinkowskiEngine's autograd (training/trainer.py:160-175: model.train(); y = model(batch);
 * loss.backward()).  Backward of a sparse convolution w.r.t. its input is again a sparse convolution on the cached
 * map (k=3: same table with kernel[26-k]^T; k=2,s=2 <-> transposed) and is composed from egonn_conv /
 * egonn_conv_transpose by the host side (egonn_amd/train.py); the entry points below are what has no forward twin.
 * `scratch`: device floats owned by the caller (partial sums of the deterministic two-stage reductions).            */
enum { EGONN_ACT_NONE = 0, EGONN_ACT_RELU = 1, EGONN_ACT_TANH = 2, EGONN_ACT_SOFTPLUS = 3, EGONN_ACT_SIGMOID = 4 };
/* Row-wise dense layer out = act(x @ Wmat + bias): weight_out_in = 0: weight (cin,cout) (ME 1x1 kernel);
 * 1: weight (cout,cin) (nn.Linear / MinkowskiLinear, models/minkgl.py:175-225).  Also the input gradient of either
 * layout (swap the flag). */
int egonn_dense(const float* x, int64_t n, int cin, const float* weight, int weight_out_in, const float* bias, int cout,
                int act, float* out, void* stream);
/* A 1x1 kernel (cin, cout multiples of 16; either layout) in the MFMA fragment order the dense kernels keep in LDS:
 *   packed[((nt * cin/16 + t) * 64 + lane) * 4 + u] = Wmat[16 t + 4 (lane >> 4) + u][16 nt + (lane & 15)]      (cin * cout floats)
 * egonn_model_finalize makes these once per model for the 1x1 convolutions of the forward; _host is the same function on host
 * memory (no device needed). */
int egonn_dense_pack_fragments(const float* weight, int weight_out_in, int cin, int cout, float* packed, void* stream);
int egonn_dense_pack_fragments_host(const float* weight, int weight_out_in, int cin, int cout, float* packed);
/* tests / measurements only: the dense launcher of the forward with everything explicit.  out[r] = act((in[r] @ Wmat + bias) * scale
 * + shift) (+ residual[r]), or with gate (B, cout) and boff (B + 1 int32 row offsets of the scans): relu(residual[r] * gate[scan of
 * r] + that).  rows_capacity sizes the grid; n_dev (nullable, device int32) is the live row count, rows from it on are not
 * written.  in / residual / out are bf16 maps where their flag is set.  form 0 = the persistent LDS kernel, 1 = its streaming
 * form (>= 8192 rows, cin in {32, 64, 128}, cout in {64, 128}, cin * cout <= 8192), which reads `packed` (nullable:
 * egonn_dense_pack_fragments of the same kernel) instead of gathering the weights.  All three compute bitwise the same rows
 * (tests/test_gpu_dense_stream.py). */
int egonn_debug_dense(const void* in, int in_bf16, int64_t rows_capacity, const int32_t* n_dev, int cin, int cout, const float* weight,
                      int weight_out_in, const float* packed, const float* bias, const float* scale, const float* shift, int act,
                      const void* residual, int res_bf16, const float* gate, const int32_t* boff, int B, void* out, int out_bf16,
                      int form, void* stream);
/* tests only, no device call: what the dense launcher picks for a layer of `rows` (capacity) x cin -> cout.  form -1 = the product
 * rule, 0 / 1 as above; gate_scans = B of a gated call, 0 = no gate.  out[0] = the kernel (0 nothing to launch, 1 streaming form,
 * 2 persistent LDS kernel, 3 small kernel, 4 64-column tile kernel, 5 thread per output), out[1], out[2] = grid x, y, out[3] =
 * dynamic LDS bytes, out[4] = output columns per block of grid y (persistent LDS kernel, else 0).  A form or a gate the shape
 * does not have is the launcher's own error. */
int egonn_debug_dense_route(int64_t rows, int cin, int cout, int form, int gate_scans, int32_t out[5]);
/* test hook, host only (no context, no device call): the whole launch sconv_map would make for one sparse-convolution layer
 * under one setting — sconv_choose, DESIGN.md §3.1 "Host side of a convolution"; tests/test_sconv_choice_host.py.
 * in = code (as egonn_debug_set_naive_conv), map kind, output level, cin, cout, bf16, gated input, split_io, epilogue residual,
 *      split level limit (-1 = exact fp32), operand autoscale, resident mask (-1 = product rule), resident max_workgroups,
 *      kparts, kw, col_parts (each -1 = the product offset-split rule; as egonn_debug_set_ksplit)
 * cap_groups = the groups the map's row-group tables hold
 * out = route, kernel (both SconvRoute of egonn_amd/csrc/kernels.h), NW, NSW, KW, KS, GATED, TRACE, resident, KSP, D, G, SPLIT,
 *       PIPE, grid x, y, z, block size, dynamic LDS bytes, kparts.  A refused combination returns the convolution's own error. */
int egonn_debug_sconv_choice(const int32_t in[16], int64_t cap_groups, int32_t out[20]);
/* out (ca,cb) = a^T b over n rows: weight gradient of a dense layer (a = input, b = grad_out for the (cin,cout) layout). */
int egonn_dense_backward_weight(const float* a, int ca, const float* b, int cb, int64_t n, float* out, float* scratch,
                                int64_t scratch_floats, void* stream);
/* Weight gradient of MinkowskiConvolution / MinkowskiConvolutionTranspose on the current plan: grad_kernel
 * (K,cin,cout).  kernel_size 5: the 1->32 input layer (in == NULL: all-ones features); 3; 2 (transposed = 0: level
 * l -> l+1, 1: l -> l-1); 1. */
int egonn_conv_backward_weight(egonn_ctx* ctx, int level_in, int level_out, int kernel_size, int transposed,
                               const float* in, int cin, const float* grad_out, int cout, float* grad_kernel,
                               float* scratch, int64_t scratch_floats, void* stream);
/* Per-channel reductions over (n,c) fp32 rows -> out (2,c) DOUBLES.  MinkowskiBatchNorm in train mode = nn.BatchNorm1d over
 * all rows (models/minkgl.py:102,107):  mode 0: sum a, sum a^2;  mode 1: sum (a-mean)^2, 0;
 * mode 2 (backward): g = a*[mask>0] (mask nullable): sum g, sum g*(b-mean);  mode 3: d = a-mean: sum d, sum d^2 (one-pass
 * statistics around a shift point, additive over ranks for SyncBN).  Differences, products and sums are fp64 throughout, so
 * the one-pass variance S2/n - (S1/n)^2 stays accurate whatever the shift (0 on a first step).  out and scratch must be
 * 8-byte aligned; scratch holds fp64 partials: >= 4*c*max(1024, ceil(n/512)) floats makes the row blocking (and so the
 * summation order) a function of n only; the minimum accepted is 4*c*ceil(n/512). */
int egonn_col_stats(int mode, const float* a, const float* b, const float* mask, const float* mean, int64_t n, int c,
                    double* out, float* scratch, int64_t scratch_floats, void* stream);
/* Per-channel BatchNorm bookkeeping of nn.BatchNorm1d in train mode, on the device:
 * forward: fp64 sums (2,c) from mode 3 around shift_point (c) over `count` rows (whole batch) -> out (4,c) = mean, invstd,
 * scale = weight*invstd, shift = bias - mean*scale; running_mean/var (nullable) updated with `momentum` (unbiased var).
 * backward: local/global fp64 (2,c) sums from mode 2 -> out (5,c) = A, B, C of egonn_affine3, dgamma, dbeta. */
int egonn_bn_train_finalize(const double* sums, const float* shift_point, double count, int c, const float* weight,
                            const float* bias, float eps, float momentum, float* running_mean, float* running_var,
                            float* out_mean_invstd_scale_shift, void* stream);
int egonn_bn_backward_finalize(const double* local_sums, const double* global_sums, double count, int c, const float* weight,
                               const float* mean, const float* invstd, float* out_abc_dgamma_dbeta, void* stream);
/* out = relu?(x*scale[c] + shift[c]) — BatchNorm application with batch statistics folded by the caller. */
int egonn_affine_act(const float* x, const float* scale, const float* shift, int64_t n, int c, int relu, float* out,
                     void* stream);
/* out = A[c]*(g*[mask>0]) + B[c]*x + C[c] — BatchNorm input gradient (mask = the ReLU output, nullable). */
int egonn_affine3(const float* g, const float* mask, const float* x, const float* A, const float* B, const float* C,
                  int64_t n, int c, float* out, void* stream);
int egonn_relu_backward(const float* grad_out, const float* out, int64_t n, int c, float* grad_in, void* stream);
/* grad_in = grad_out * act'(.) from the activation's output (MinkowskiReLU / Tanh / Softplus / Sigmoid,
 * models/minkgl.py:181-183,198-200). */
int egonn_act_backward(int act, const float* grad_out, const float* out, int64_t n, int c, float* grad_in, void* stream);
/* MinkowskiFunctional.normalize = F.normalize(x, p=2, dim=1, eps=1e-12) (models/minkgl.py:222-223): grad_out == NULL:
 * out = normalised rows; else out = the input gradient for grad_out. */
int egonn_l2_normalize(const float* x, const float* grad_out, int64_t n, int c, float* out, void* stream);
/* ECALayer gate on the (B, channels) per-sample means: gate = sigmoid(Conv1d(1,1,k,padding=(k-1)/2,bias=False)(mean))
 * (layers/eca_block.py:17-19,28-31) and its backward (grad_mean (B,channels), grad_weight (k,), fixed-order sums). */
int egonn_eca_gate(const float* mean, const float* conv_weight, int kernel_size, int batch_size, int channels, float* gate,
                   void* stream);
int egonn_eca_gate_backward(const float* grad_gate, const float* gate, const float* mean, const float* conv_weight,
                            int kernel_size, int batch_size, int channels, float* grad_mean, float* grad_weight,
                            void* stream);
/* SELayer gate on the (B, channels) per-sample means (layers/senet_block.py:34-50, block :53-89, selected by
 * `block = SEBasicBlock`, models/minkloc.py:30-31): gate = sigmoid(W2 relu(W1 mean_b + b1) + b2), the fc Sequential of two
 * MinkowskiLinear layers (:39-43) with w1 (hidden,channels), w2 (channels,hidden) in nn.Linear layout.  channels a multiple
 * of 16 in 16..256, hidden = channels/16 (reduction = 16); anything else is EGONN_STATUS_INVALID.  hidden_out (nullable):
 * (B,hidden) post-ReLU activations, what the backward needs.  Backward: ReLU by hidden_act > 0; grad_mean (B,channels),
 * grad_w1/b1/w2/b2 in the parameters' shapes, each a serial sum over the samples in order (bitwise reproducible, no atomics).
 * One launch each, no host sync.  The block tail around it is egonn_global_avg_pool + egonn_gate_residual(relu = 1). */
int egonn_se_gate(const float* mean, const float* w1, const float* b1, const float* w2, const float* b2, int batch_size,
                  int channels, int hidden, float* gate, float* hidden_out, void* stream);
int egonn_se_gate_backward(const float* grad_gate, const float* gate, const float* hidden_act, const float* mean,
                           const float* w1, const float* w2, int batch_size, int channels, int hidden, float* grad_mean,
                           float* grad_w1, float* grad_b1, float* grad_w2, float* grad_b2, void* stream);
/* out = relu?(x * gate[sample] + residual): MinkowskiBroadcastMultiplication + residual add + MinkowskiReLU
 * (layers/eca_block.py:69-73) with an explicit (B,c) gate (nullable = 1); backward: d = grad_out*[out>0],
 * grad_residual = d (nullable), grad_x = d*gate. */
int egonn_gate_residual(egonn_ctx* ctx, int level, const float* x, const float* gate, const float* residual, int channels,
                        int relu, float* out, void* stream);
int egonn_gate_residual_backward(egonn_ctx* ctx, int level, const float* grad_out, const float* out, const float* gate,
                                 int channels, float* grad_x, float* grad_residual, void* stream);
/* Per-sample column sums -> out (B,c).  mode 0: a*b;  mode 1: t^p ln t, t = max(a,1e-6) (GeM d/dp);
 * mode 2: (a*[b>0])*x2 (gate gradient).  scratch >= 32*B*c floats. */
int egonn_segment_sums(egonn_ctx* ctx, int level, int mode, const float* a, const float* b, const float* x2,
                       const float* p, int channels, float* out, float* scratch, int64_t scratch_floats, void* stream);
/* out[r] = v[sample(r)] (* 1/n_sample when mean): backward of MinkowskiGlobalPooling (layers/eca_block.py:16). */
int egonn_segment_broadcast(egonn_ctx* ctx, int level, const float* v, int channels, int mean, float* out, void* stream);
/* GeM input gradient: grad_x[r] = coef[sample(r)] * x^(p-1) * [x >= 1e-6] (layers/pooling.py:82-86). */
int egonn_gem_backward(egonn_ctx* ctx, int level, const float* x, const float* coef, const float* p, int channels,
                       float* grad_x, void* stream);

/* ------------------------------------------------------------------ scan ingest (the step before the path)
 * replaces PointCloudLoader.__call__ (misc/point_clouds.py:95-111) after read_pc (datasets/mulran/mulran_raw.py:19-25,
 * datasets/kitti/kitti_raw.py:16-22): raw (n, floats_per_point = 4 | 3) f32 returns of a whole batch (scan b = rows
 * [scan_offsets[b], scan_offsets[b+1]), DEVICE int64, batch_size+1 entries); drops all-zero points (|v| <= 1e-8) and
 * points with z <= ground_plane_level; survivors keep their order.  out_points (n,3) f32 (first out_scan_offsets[B]
 * rows valid), out_scan_offsets (batch_size+1) DEVICE int64.  scratch: egonn_filter_points_scratch_ints(n) int32.
 * n is a CAPACITY (>= scan_offsets[batch_size]; rows beyond scan_offsets[batch_size] are never read; with n == 0 raw
 * may be NULL), so that a fixed-size launch sequence serves every batch (hipGraph capture).  No host sync:
 * out_scan_offsets can be handed to egonn_voxelize_device as they are (egonn_amd/stream.py), or copied back for
 * egonn_voxelize. */
int64_t egonn_filter_points_scratch_ints(int64_t n);
int egonn_filter_points(const float* raw, int64_t n, int floats_per_point, const int64_t* scan_offsets, int batch_size,
                        int remove_zero_points, int remove_ground_plane, float ground_plane_level, float* out_points,
                        int64_t* out_scan_offsets, int32_t* scratch, int64_t scratch_ints, void* stream);

/* ------------------------------------------------------------------ retrieval (database build, configs[4])
 * replaces the per-query NumPy search of Evaluator.evaluate, eval/evaluate.py:80-82 and :175-176:
 *   embed_dist = np.linalg.norm(map_embeddings - query_embedding, axis=1);  nn_ndx = np.argsort(embed_dist)[:k]
 * out_index (n_query,k) int32 ascending by distance (ties: lower index; -1 beyond n_database), out_distance (n_query,k).
 * +inf distances (an infinite or overflowing element) sort after every finite one, in index order; a NaN distance is never
 * a neighbour: such rows are left out and the list ends with (-1, +inf).  scratch >= n_query*n_database floats. */
int egonn_knn(const float* query, int64_t n_query, const float* database, int64_t n_database, int dim, int k,
              int32_t* out_index, float* out_distance, float* scratch, int64_t scratch_floats, void* stream);
/* eval/evaluate.py:84-88 / :181-184: out_true_positives (n_radius,k) int32, [r][nn] = number of queries with a
 * retrieved map element among the first nn+1 whose position is within radius[r] (positions: (n, position_dim) f32). */
int egonn_recall_counts(const int32_t* nn_index, const float* query_positions, const float* map_positions,
                        int64_t n_query, int k, int position_dim, const float* radius, int n_radius,
                        int32_t* out_true_positives, void* stream);

/* ------------------------------------------------------------------ 6-DoF registration of keypoint sets (local evaluation)
 * replaces get_ransac_result (eval/evaluate.py:381-399; called by ransac_fn :296-306), calculate_repeatability (:402-411)
 * and the RRE / RTE / success arithmetic (:245-252).  The reference hands the estimation to Open3D's
 * registration_ransac_based_on_feature_matching, which is not part of the reference tree: its behaviour is restated from
 * its documentation [recall] (egonn_amd/csrc/registration.hip spells out every rule, the draw function included).
 * Two deliberate differences: all n_hypotheses hypotheses are evaluated (Open3D stops early by its 0.999 confidence rule),
 * and a draw is a pure function of (seed, pair id, hypothesis, slot) (Open3D's generator depends on its threads), so
 * results are bitwise reproducible, independent of the batch a pair sits in and of the launch geometry.
 *
 * Batched over n_pairs independent (source = query, target = candidate) pairs, padded to n_max <= 256 rows per side:
 * feat (n_pairs, n_max, dim) f32 with dim a multiple of 4 up to 256 (16-byte aligned), kp (n_pairs, n_max, 3) f32, per-pair
 * row counts n1 / n2 (n_pairs) DEVICE int32 (clipped to [0, n_max] on the device and reported).  No host synchronisation.
 * pair_id (n_pairs) DEVICE int32, nullable: the id that enters the draws (null = the pair's index in the batch).  Only its
 * low 30 bits are used (0 <= pair_id < 2^30; n_hypotheses < 2^31): ids that agree in them draw the same samples.
 * Geometry is fp64 throughout. */
enum { EGONN_REG_STATUS_CLIPPED = 1,      /* a count was outside [0, n_max] and was clipped */
       EGONN_REG_STATUS_FEW_CORR = 2,     /* fewer than 3 correspondences */
       EGONN_REG_STATUS_NO_MODEL = 4,     /* no hypothesis passed the checks with an inlier: T = identity, 0 inliers */
       EGONN_REG_STATUS_BAD_INDEX = 8 };  /* a correspondence index outside its set (clamped) */
/* bytes of the scratch that carries the per-workgroup bests from egonn_ransac_pairs to egonn_registration_finish
 * (-1 on bad arguments) */
int64_t egonn_registration_scratch_bytes(int n_pairs, int n_max, int n_hypotheses);
/* correspondences by mutual nearest neighbours in descriptor space (csrc/match.hip): ONE operator with two addressings,
 * egonn_match_mutual (dense: pair p = block p of both sides) and egonn_match_candidates below (indexed: side 2 of pair p is
 * the bank block nn_index names).  Both run the same two kernels and give the same bits on the same operands.  fp64 squared
 * L2 of the exactly converted fp32 inputs, k ascending, one fma per term: j(i) = nearest target of source i, i(j) = nearest
 * source of target j, ties: lowest index; keep (i, j(i)) iff i(j(i)) == i; fewer than 3 such pairs: every (i, j(i)).
 * corr (n_pairs, n_max, 2) int32 compacted in ascending i (unused rows -1), n_corr (n_pairs).  Each distance is computed
 * once, by workgroups of 64 source rows x 32 target rows whose partial minima go to the caller's scratch (8-byte aligned,
 * egonn_match_mutual_scratch_bytes: (cdiv(n_max, 64) + cdiv(n_max, 32)) * n_max * 12 bytes per pair, -1 on bad arguments)
 * and are merged in ascending tile order. */
int64_t egonn_match_mutual_scratch_bytes(int n_pairs, int n_max);
int egonn_match_mutual(const float* feat1, const float* feat2, const int32_t* n1, const int32_t* n2, int n_pairs, int n_max,
                       int dim, int32_t* corr, int32_t* n_corr, void* scratch, int64_t scratch_bytes, void* stream);
/* hypotheses t = 0 .. n_hypotheses-1 of every pair: 3 drawn correspondences, degeneracy / edge-length (0.8) / distance
 * (dist_th) checks, the rigid transform of the 3 pairs (no scale, reflection corrected), then over all correspondences
 * inlier iff |T s_i - t_j| < dist_th.  Writes each workgroup's best (inliers, sum of squared inlier distances, t) to scratch.
 * Optional debug tables (null = not written): hyp_count (n_pairs, n_hypotheses) int32 = inliers, or -1 degenerate draw,
 * -2 edge check, -3 distance check; hyp_err2 (n_pairs, n_hypotheses) f64 = sum of squared inlier distances. */
int egonn_ransac_pairs(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* corr,
                       const int32_t* n_corr, const int32_t* pair_id, int n_pairs, int n_max, int n_hypotheses, uint64_t seed,
                       double dist_th, void* scratch, int64_t scratch_bytes, int32_t* hyp_count, double* hyp_err2, void* stream);
/* best hypothesis = most inliers, then smallest squared-distance sum (lowest rmse), then lowest t; its transform T
 * (n_pairs,4,4) f64 row-major in the caller's coordinates; then the final evaluation, which is what the reference's
 * len(correspondence_set) counts: every source keypoint under T whose nearest target keypoint is closer than dist_th ->
 * inliers (n_pairs) int32, fitness = inliers / n1, inlier_rmse (f64), corr_set (n_pairs, n_max, 2) int32 (nullable; unused
 * rows -1), best_t (nullable; -1 = none).  Same corr / pair_id / n_hypotheses / seed / dist_th / scratch as the
 * egonn_ransac_pairs call before it.  With T_gt (n_pairs,4,4) f64 (nullable): rte = |t_est - t_gt|, rre in degrees =
 * acos(clip((trace(R_est^T R_gt) - 1) / 2)), success = rte <= 2 and rre <= 5, repeatability = share of source keypoints with a
 * target keypoint within repeat_th under T_gt (the transform applied in fp64; the reference applies it in fp32).  status
 * (n_pairs) int32 of EGONN_REG_STATUS_* bits (nullable); a pair without a model is not an error of the call.
 * corr == NULL: nothing is estimated, only repeatability under T_gt is written (calculate_repeatability on its own). */
int egonn_registration_finish(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* corr,
                              const int32_t* n_corr, const int32_t* pair_id, int n_pairs, int n_max, int n_hypotheses,
                              uint64_t seed, double dist_th, const void* scratch, int64_t scratch_bytes, const double* T_gt,
                              double repeat_th, double* T, int32_t* inliers, double* fitness, double* inlier_rmse,
                              int32_t* corr_set, int32_t* best_t, double* rte, double* rre, int32_t* success,
                              double* repeatability, int32_t* status, void* stream);
/* Spectral geometric verification (csrc/spectral.hip): the hypothesis-free counterpart of egonn_ransac_pairs +
 * egonn_registration_finish on the same operands (kp1, kp2, n1, n2, corr, n_corr as above; no pair id, no seed).  Per pair,
 * with m = n_corr and (p_i, q_i) = (kp1[corr[i][0]], kp2[corr[i][1]]) converted exactly to fp64:
 *   M_ij = max(0, 1 - d_ij^2 / d_thr^2), d_ij = | |p_i - p_j| - |q_i - q_j| |, M_ii = 0 (fp64, stored rounded to fp32);
 *   v = 1 / sqrt(m) everywhere, then exactly `iterations` times u = M v; |u| = 0: stop; v = u / |u|;  eigenvalue = v^T M v
 *   (about the size of the mutually consistent set minus 1; fp64 sums in a fixed order: a row in ascending j, the rows by a
 *   64-lane butterfly and then ascending waves);  score = eigenvalue / (n_max - 1), the normaliser fixed so that a pair with
 *   few correspondences cannot outrank one with many consistent ones (0 when n_max = 1);
 *   seeds S = { i : v_i >= seed_ratio * max v };  T0 = least-squares rigid transform of S (no scale, det +1: Horn's closed form
 *   with the fixed-schedule Jacobi of the ICP);  I = { i : |T0 p_i - q_i| < dist_th };  T = the rigid transform of I.
 * inliers, fitness, inlier_rmse, corr_set and, with T_gt, rte / rre / success / repeatability are then those of
 * egonn_registration_finish under T: same definitions, shapes and dtypes, so egonn_pick_candidates consumes them unchanged.
 * status: CLIPPED / BAD_INDEX as the registration; FEW_CORR when m < 3; NO_MODEL when M = 0, |S| < 3, |I| < 3 or a fit is
 * degenerate (coincident or collinear points: a scatter matrix C with e2(C) <= 1e-10 tr(C)^2, e2 = the sum of its principal
 * 2 x 2 minors); in both cases T = identity and 0 inliers.  No output is ever NaN for finite keypoints inside the counts.
 * eigenvalue, score (n_pairs) f64, weights (n_pairs, n_max) f64 = v, zero from m on, n_seeds (n_pairs) int32 = |S|.  Every
 * output is nullable (null = not written).  Rows of corr from n_corr on and keypoints beyond the counts are never read.
 * d_thr > 0, iterations >= 1, 0 < seed_ratio <= 1, dist_th > 0 (checked, with the shape and the pointers, before anything is
 * launched).  One launch, no host synchronisation, no float atomics: deterministic, capturable, and a pair's result does not
 * depend on n_pairs, on its position in the batch or on other pairs.  scratch: egonn_spectral_verify_scratch_bytes
 * (n_pairs, n_max) bytes, 8-byte aligned: 0 (scratch may be null) up to n_max = 128, where M lives in LDS, else
 * min(n_pairs, 512) * n_max^2 * 4 for the workgroups' slabs of M; -1 on bad arguments. */
int64_t egonn_spectral_verify_scratch_bytes(int n_pairs, int n_max);
int egonn_spectral_verify(const float* kp1, const float* kp2, const int32_t* n1, const int32_t* n2, const int32_t* corr,
                          const int32_t* n_corr, int n_pairs, int n_max, double d_thr, int iterations, double seed_ratio,
                          double dist_th, const double* T_gt, double repeat_th, void* scratch, int64_t scratch_bytes,
                          double* eigenvalue, double* score, double* weights, int32_t* n_seeds, double* T, int32_t* inliers,
                          double* fitness, double* inlier_rmse, int32_t* corr_set, double* rte, double* rre, int32_t* success,
                          double* repeatability, int32_t* status, void* stream);

/* ------------------------------------------------------------------ ICP refinement of scan pairs (local evaluation, tuples)
 * replaces icp() of misc/point_clouds.py:31-62 (voxel_down_sample(0.1) of both clouds, then Open3D's registration_icp,
 * point-to-point, ICPConvergenceCriteria(max_iteration)); called by eval/evaluate.py:215-236 and
 * datasets/mulran/generate_training_tuples.py:83.  Open3D is not part of the reference tree: the rules are restated from
 * its documentation [recall] (egonn_amd/csrc/icp.hip).  Deliberate differences: the downsampled order is fixed
 * (ascending voxel index), and the source is always transformed from the original points by the cumulative transform.
 * All geometry is fp64; results are bitwise reproducible and independent of the batch a pair sits in. */
enum { EGONN_ICP_STATUS_FEW_CORR = 1,     /* a round met fewer than 3 correspondences: the loop stopped with T unchanged */
       EGONN_ICP_STATUS_MAX_ITER = 2,     /* stopped by the round limit */
       EGONN_ICP_STATUS_EMPTY = 4,        /* a side has no points: T = init, fitness 0 */
       EGONN_ICP_STATUS_RANGE = 8 };      /* downsample: a voxel index needs more than 21 bits (or a non-finite point) */
/* Voxel-grid downsample of n_clouds clouds: points (n,3) f32 concatenated, cloud c = rows [offsets[c], offsets[c+1]) (DEVICE
 * int64, n_clouds+1; n is a CAPACITY as in egonn_filter_points).  crop: 6 HOST floats min_x, max_x, min_y, max_y, min_z,
 * max_z (nullable; NaN = no bound): keep x > min_x and x <= max_x, likewise y, z (preprocess_pointcloud,
 * datasets/dataset_utils.py:235-265).  mb = min over the kept points - voxel_size/2 per axis; idx = floor((p - mb) /
 * voxel_size); one output point per occupied voxel = fp64 mean of its points summed in input order, in ascending (ix, iy,
 * iz).  out_points (n,3) f64 (first out_offsets[n_clouds] rows valid), out_offsets (n_clouds+1) DEVICE int64, out_counts (n)
 * int32 points per voxel (nullable), status (n_clouds) DEVICE int32: EGONN_ICP_STATUS_RANGE = nothing written for that
 * cloud.  scratch: egonn_voxel_downsample_scratch_bytes(n, n_clouds) bytes (-1 on bad arguments), 256-byte aligned.
 * No host synchronisation. */
int64_t egonn_voxel_downsample_scratch_bytes(int64_t n, int n_clouds);
int egonn_voxel_downsample(const float* points, int64_t n, const int64_t* offsets, int n_clouds, double voxel_size,
                           const float* crop, double* out_points, int64_t* out_offsets, int32_t* out_counts, int32_t* status,
                           void* scratch, int64_t scratch_bytes, void* stream);
/* Point-to-point ICP of n_pairs independent (source, target) pairs: src (n_src,3) / tgt (n_tgt,3) f64 with DEVICE int64
 * offsets (n_pairs+1 each; n_src / n_tgt are capacities), T_init (n_pairs,4,4) f64 (nullable = identity).
 * Evaluation under T: j(i) = nearest target point of T s_i (fp64 squared distance, ties: lowest index), a correspondence iff
 * the distance is < max_dist; fitness = n_corr / n_source; inlier_rmse = sqrt(sum d2 / n_corr) (0 without correspondences).
 * A squared distance that is not finite never wins: a source or target row with a NaN or an infinite coordinate is never part
 * of a correspondence and is never counted, and every other row is evaluated as if that row held no point.
 * T_0 = init is evaluated; round k: U = least-squares rigid transform (no scale, det +1) of {T_k s_i} onto {t_j(i)},
 * T_k+1 = U T_k, evaluated; the loop stops after that evaluation if |d fitness| < eps_fitness and |d rmse| < eps_rmse, after
 * max_iteration rounds (MAX_ITER), or before a round with fewer than 3 correspondences (FEW_CORR, T unchanged).
 * Outputs: T (n_pairs,4,4) f64, fitness, inlier_rmse (n_pairs) f64 of the last evaluation, iterations (rounds run), status
 * (EGONN_ICP_STATUS_* bits), all (n_pairs).  Nullable debug tables: T_trace (n_pairs, max_iteration+1, 4, 4) = T_k (zero
 * beyond the last), eval_trace (n_pairs, max_iteration+1, 3) = (n_corr, sum d2, stop flag) of evaluation k, corr (n_src)
 * int32 = j(i) of the last evaluation (index inside the pair's target) or -1.
 * The call enqueues a fixed launch sequence for max_iteration rounds; a stopped pair's later launches return at once: no host
 * synchronisation, capturable.  scratch: egonn_icp_scratch_bytes(n_src, n_tgt, n_pairs) bytes (-1 on bad arguments),
 * 256-byte aligned. */
int64_t egonn_icp_scratch_bytes(int64_t n_src, int64_t n_tgt, int n_pairs);
int egonn_icp_pairs(const double* src, int64_t n_src, const int64_t* src_offsets, const double* tgt, int64_t n_tgt,
                    const int64_t* tgt_offsets, int n_pairs, const double* T_init, double max_dist, int max_iteration,
                    double eps_fitness, double eps_rmse, double* T, double* fitness, double* inlier_rmse, int32_t* iterations,
                    int32_t* status, double* T_trace, double* eval_trace, int32_t* corr, void* scratch, int64_t scratch_bytes,
                    void* stream);

/* ------------------------------------------------------------------ point-to-plane ICP: surface normals and the 6-DoF solve
 * the other estimator of icp() (misc/point_clouds.py:31-62, point2plane=True): estimate_normals(KDTreeSearchParamKNN(knn=20))
 * on the downsampled clouds, then registration_icp with TransformationEstimationPointToPlane.  Restated from Open3D's
 * documentation [recall] like the block above.  Deliberate difference: only the TARGET's normals are computed, point-to-plane
 * never reads the source's.  fp64, no floating-point atomics, fixed summation orders: a cloud's or pair's result has the same
 * bits alone, in any batch and at any batch position. */
enum { EGONN_ICP_STATUS_SINGULAR = 16 };  /* plane: a pivot of the 6 x 6 solve is not > 2^-40 of A's diagonal entry, or the
                                           * step is not finite (one plane, a corridor): the loop stopped with T unchanged */
enum { EGONN_NORMALS_STATUS_FEW_POINTS = 1,   /* the cloud has fewer than knn points: every list holds the whole cloud */
       EGONN_NORMALS_STATUS_RANGE = 2 };      /* a non-finite coordinate: every normal of the cloud is (0,0,1) */
/* Surface normals of n_clouds resident clouds: points (n,3) f64 concatenated (the layout egonn_voxel_downsample returns; n is
 * a CAPACITY), DEVICE int64 offsets (n_clouds+1), knn in [3, 32].
 * Neighbours of a point: all points of the same cloud, itself included, ordered by (d2, index) ascending with
 * d2 = (dx*dx + dy*dy) + dz*dz; the first m = min(knn, cloud size) are taken (an exact search).  mean = (sum q) / m and
 * C = sum (q - mean)(q - mean)^T / m, both summed in neighbour order.  The normal is the unit eigenvector of C's smallest
 * eigenvalue (cyclic Jacobi, fixed schedule), flipped so that n . p <= 0 (toward the sensor at the origin of the cloud's
 * frame); if n . p == 0 its first non-zero component is positive.  m < 3, a largest eigenvalue that is not > 0 or a non-finite
 * value gives (0,0,1).
 * Outputs: normals (n,3) f64, status (n_clouds) DEVICE int32 (EGONN_NORMALS_STATUS_* bits).  Nullable debug tables: neighbors
 * (n, knn) int32 = index inside the cloud in the order above, -1 beyond m (all -1 in a RANGE cloud); eigenvalues (n,3)
 * ascending (0 in a RANGE cloud).  Rows outside every cloud are not written.
 * scratch: egonn_estimate_normals_scratch_bytes(n, n_clouds) bytes (-1 on bad arguments), 256-byte aligned.  No host
 * synchronisation, capturable. */
int64_t egonn_estimate_normals_scratch_bytes(int64_t n, int n_clouds);
int egonn_estimate_normals(const double* points, int64_t n, const int64_t* offsets, int n_clouds, int knn, double* normals,
                           int32_t* status, int32_t* neighbors, double* eigenvalues, void* scratch, int64_t scratch_bytes,
                           void* stream);
/* Point-to-plane ICP: the arguments of egonn_icp_pairs plus tgt_normals (n_tgt,3) f64 (required; what egonn_estimate_normals
 * returns for tgt).  The evaluation (nearest target by POINT distance, strict < max_dist, fitness and rmse from point
 * distances), the stop rule and the trace tables are those of egonn_icp_pairs.  Round k: for each correspondence (i, j)
 * vs = T_k s_i, r = (vs - t_j) . n_j, J = [vs x n_j, n_j]; A = sum J J^T, b = sum J r; A x = -b by LDL^T without pivoting;
 * U = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)]; T_k+1 = U T_k.  Before a round: fewer than 6 correspondences stop the loop with
 * FEW_CORR, a pivot d_i that is not > 2^-40 A_ii or a non-finite x with SINGULAR, T unchanged in both cases.
 * scratch: egonn_icp_plane_scratch_bytes(n_src, n_tgt, n_pairs) bytes (-1 on bad arguments), 256-byte aligned. */
int64_t egonn_icp_plane_scratch_bytes(int64_t n_src, int64_t n_tgt, int n_pairs);
int egonn_icp_plane_pairs(const double* src, int64_t n_src, const int64_t* src_offsets, const double* tgt, int64_t n_tgt,
                          const int64_t* tgt_offsets, const double* tgt_normals, int n_pairs, const double* T_init, double max_dist,
                          int max_iteration, double eps_fitness, double eps_rmse, double* T, double* fitness, double* inlier_rmse,
                          int32_t* iterations, int32_t* status, double* T_trace, double* eval_trace, int32_t* corr, void* scratch,
                          int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ training augmentation of a resident scan batch
 * replaces TrainTransform (datasets/augmentation.py:10-30, called per scan by datasets/base_datasets.py:70-76),
 * TrainSetTransform (:33-48, called per batch by datasets/dataset_utils.py:67-72) and the rigid perturbation of the local
 * phase (datasets/mulran/mulran_train.py:41-50) for scans that are already on the device.  Capacity-based and free of host
 * synchronisation like egonn_filter_points, so it can sit in front of egonn_voxelize_device inside a captured graph.
 * egonn_amd/csrc/augment.hip spells out every rule, the deliberate differences and the draw: a draw is a pure function of
 * (seed, draw, scan id, point index, slot) through splitmix64, so a scan's augmentation does not depend on its batch. */
enum { EGONN_AUG_JITTER = 1, EGONN_AUG_REMOVE_POINTS = 2, EGONN_AUG_TRANSLATE = 4, EGONN_AUG_ROTATE = 8, EGONN_AUG_BLOCK = 16,
       EGONN_AUG_SET_ROTATE = 32, EGONN_AUG_FLIP = 64, EGONN_AUG_RIGID = 128, EGONN_AUG_JITTER_CLIP = 256, EGONN_AUG_ALL = 511 };
enum { EGONN_AUG_STATUS_BAD_ID = 1 };     /* scan id outside [0, 2^22) (or a scan of 2^24 - 2 points or more): its points are NaN */
typedef struct egonn_augment_params {
  uint64_t seed;
  uint32_t draw;            /* draw counter, e.g. the epoch: < 2^14 */
  uint32_t set_id;          /* id of the batch's own draw (stage 2): < 2^22 */
  uint32_t stages;          /* EGONN_AUG_* bits: every stage is switched on its own */
  uint32_t reserved;
  double sigma, clip;                 /* JitterPoints (clip used with EGONN_AUG_JITTER_CLIP) */
  double r_min, r_max;                /* RemoveRandomPoints */
  double max_delta;                   /* RandomTranslation */
  double max_theta;                   /* RandomRotation about z, degrees (stage 1) */
  double block_p, scale_lo, scale_hi, ratio_lo, ratio_hi;   /* RemoveRandomBlock */
  double set_max_theta;               /* RandomRotation about z, degrees (stage 2) */
  double flip_cum[3];                 /* RandomFlip: cumulative sums of p */
  double rot_max, trans_max;          /* rigid perturbation: radians, metres */
} egonn_augment_params;
/* points (n,3) f32, scan b = rows [scan_offsets[b], scan_offsets[b+1]) (DEVICE int64, batch_size+1; n < 2^24 is a CAPACITY:
 * rows beyond scan_offsets[batch_size] are neither read nor written); scan_ids (batch_size) DEVICE int32, nullable = the
 * position in the batch; out_points (n,3) f32 (may be points itself).  T_in / T_out (batch_size,4,4) f32 row-major, both
 * nullable: T_out = m @ T_in with m the rigid perturbation of the scan (T_in null = identity).  Optional outputs (null =
 * not written): rec_i (batch_size,8) int32 = n, k removed, block drawn, flip axis (-1 none), status bits, scan id, low and
 * high word of the removal threshold key; rec_d (batch_size,32) f64 = [0] r, [1..3] translation, [4..6] theta, cos, sin
 * of stage 1, [7] block u, [8..13] box min xyz, max xyz, [14..19] block x, y, w, h, x + w, y + h, [20..23] set theta, cos,
 * sin, flip u, [24..28] rigid angle, cos, sin, tx, ty, [29] erase area, [30] aspect ratio (fields of stages that are off
 * or not drawn are 0; translation, cos and sin are the fp64 values BEFORE their one rounding to fp32, the box and the block
 * are fp32 values); flags (n) uint8: bit 0 = removed by RemoveRandomPoints, bit 1 = erased by RemoveRandomBlock.
 * scratch: egonn_augment_scratch_bytes(n, batch_size) bytes (-1 on bad arguments), 256-byte aligned. */
int64_t egonn_augment_scratch_bytes(int64_t n, int batch_size);
int egonn_augment_points(const float* points, int64_t n, const int64_t* scan_offsets, int batch_size, const int32_t* scan_ids,
                         const egonn_augment_params* params, const float* T_in, float* out_points, float* T_out,
                         int32_t* rec_i, double* rec_d, uint8_t* flags, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ ScanContext baseline (hand-crafted descriptor)
 * replaces third_party/scan_context/scan_context.py: ScanContext.__call__ (:9-55), sc2rk (:86-88), distance_sc (:58-83) and the
 * rerank of ScanContextManager.query (:145-154); evaluate_scan_context.py:24-84 is built on these plus egonn_knn over the ring
 * keys and egonn_recall_counts (egonn_amd/scan_context.py).  Supported shapes: 1 <= num_ring <= 40, 2 <= num_sector <= 128,
 * rerank 1 <= k <= 128.  No host synchronisation, no float atomics: every result is bitwise reproducible and independent of
 * the batch an item sits in; every call can be captured into a graph.
 *
 * Descriptor: points (n,3) f32, scan b = rows [scan_offsets[b], scan_offsets[b+1]) (DEVICE int64, batch_size+1; n is a
 * CAPACITY as in egonn_filter_points).  In float32, as the reference computes on float32 arrays: theta = clip(atan2(y,x) +
 * pi, 0, 2pi - 1e-6), ring = floor(|(x,y)| / (max_length / num_ring)), sector = floor(theta / (2pi / num_sector)) (both the
 * floor of the exact quotient of the float32 operands, which is what numpy's floor-division gives); points with ring >=
 * num_ring or a NaN coordinate are dropped; cell = max(0, max over its points of z + lidar_height), an empty cell +0.0.
 * out_sc (batch_size, num_ring, num_sector) f32, out_ringkey (batch_size, num_ring) f32 (nullable) = the row means. */
int egonn_scan_context(const float* points, int64_t n, const int64_t* scan_offsets, int batch_size, int num_sector,
                       int num_ring, double max_length, double lidar_height, float* out_sc, float* out_ringkey, void* stream);
/* sc2rk on its own: sc (n, num_ring, num_sector) f32 -> out_ringkey (n, num_ring), the mean over sectors in a fixed order */
int egonn_scan_context_ringkey(const float* sc, int64_t n, int num_ring, int num_sector, float* out_ringkey, void* stream);
/* distance_sc(map_sc[c], query_sc[q]) for c = candidates[q][j] (DEVICE int32 (n_query, k); NULL = every map element, k =
 * n_map): for shift i = 1..S, a = roll(candidate, i) along the sectors, sim_i = mean over the columns whose norm exceeds 1e-8
 * on both sides of the column cosine; out_dist = 1 - max_i sim_i, out_yaw = (argmax_i + 1) % S with the first maximum in
 * shift order 1..S (the identity shift i = S loses ties) and, as np.argmax / np.max have it, NaN as the maximum: a pair with
 * an all-zero descriptor gives (NaN, 1).  A candidate outside [0, n_map) gives (+inf, -1).  fp32 arithmetic. */
int egonn_scan_context_distance(const float* query_sc, int64_t n_query, const float* map_sc, int64_t n_map, int num_ring,
                                int num_sector, const int32_t* candidates, int k, float* out_dist, int32_t* out_yaw,
                                void* stream);
/* every query's k entries ascending by distance, NaN after every number (np.argsort), equal distances by lower candidate
 * index then lower position.  candidates nullable (= the position).  Outputs must not alias inputs. */
int egonn_scan_context_rerank(const float* dist, const int32_t* yaw, const int32_t* candidates, int64_t n_query, int k,
                              int32_t* out_index, float* out_dist, int32_t* out_yaw, void* stream);

/* ------------------------------------------------------------------ training tuples (egonn_amd/csrc/tuples.hip)
 * What datasets/mulran/generate_training_tuples.py, filter_query_elements (datasets/dataset_utils.py:210-232) and the mask
 * loops of make_collate_fn (:83-88) do around the ICP, on the device.  All geometry is fp64 with contraction off, there are no
 * float atomics, every result is bitwise reproducible, and no entry synchronises with the host. */
enum { EGONN_TUPLES_STATUS_CAPACITY = 1,     /* an output did not fit its capacity: nothing was written past it */
       EGONN_TUPLES_STATUS_BAD_OFFSETS = 2,  /* row offsets that are not the exclusive scan of the counts / not inside their table */
       EGONN_TUPLES_STATUS_BAD_INDEX = 4 };  /* a label or a pick outside its table */
enum { EGONN_POSE_STATUS_BAD_ROW = 1,        /* a pose whose last row is not exactly 0 0 0 1 */
       EGONN_POSE_STATUS_SINGULAR = 2,       /* det R_b is zero or not finite */
       EGONN_POSE_STATUS_BAD_INDEX = 4 };    /* idx_a or idx_b outside [0, n_poses) */
/* Radius join of 2-D positions: query (nq,2) and ref (nm,2) f64 on the DEVICE, nq, nm <= 2^24.  j is a neighbour of i iff
 *     dx = qx_i - mx_j;  dy = qy_i - my_j;  dx*dx + dy*dy <= r*r        (each operation rounded to fp64)
 * which is what sklearn's KDTree.query_radius returns on the same positions (tests/golden/make_golden_tuples.py asserts it
 * row by row).  A NaN coordinate is never a neighbour and has none.  radii: 1 to 4 HOST doubles, finite, >= 0.
 * exclude_self (bit r of exclude_self_mask = radius r) drops j == i and nothing else; it is legal only when query and ref are
 * the same array (same pointer, nq == nm).
 * count: counts (n_radius, nq) int32.  fill: one radius; offsets (nq+1) DEVICE int64 = the exclusive scan of that radius'
 * counts; writes the neighbours of row i to indices[offsets[i] .. offsets[i+1]) in ASCENDING order (no sort: the order is by
 * construction).  capacity = entries `indices` can hold: a hit whose slot is beyond it is dropped and sets
 * EGONN_TUPLES_STATUS_CAPACITY in the DEVICE int32 *status (cleared by the call); offsets that disagree with the counts set
 * EGONN_TUPLES_STATUS_BAD_OFFSETS and nothing is written outside a row. */
int egonn_radius_count(const double* query, int64_t nq, const double* ref, int64_t nm, const double* radii, int n_radius,
                       int exclude_self_mask, int32_t* counts, void* stream);
int egonn_radius_fill(const double* query, int64_t nq, const double* ref, int64_t nm, double radius, int exclude_self,
                      const int64_t* offsets, int32_t* indices, int64_t capacity, int32_t* status, void* stream);
/* The (B,B) masks of a batch from the two CSR tables of the tuples (offsets (n_tuples+1) DEVICE int64, indices DEVICE int32
 * sorted inside a row, n_pos / n_non = entries of the index arrays): with l = labels (B) DEVICE int32,
 *     positives_mask[i][j] = l[j] in positives[l[i]],   negatives_mask[i][j] = l[j] not in non_negatives[l[i]]
 * as uint8 0/1, each membership a binary search (in_sorted_array, datasets/dataset_utils.py:270-275).  A label outside
 * [0, n_tuples) sets EGONN_TUPLES_STATUS_BAD_INDEX in *status (DEVICE int32, cleared by the call) and its row and column are 0
 * in both masks.  batch_size <= 4096.  One memset + one launch: capturable. */
int egonn_pair_masks(const int32_t* labels, int batch_size, const int64_t* pos_offsets, const int32_t* pos_indices, int64_t n_pos,
                     const int64_t* non_offsets, const int32_t* non_indices, int64_t n_non, int64_t n_tuples,
                     uint8_t* positives_mask, uint8_t* negatives_mask, int32_t* status, void* stream);
/* out[p] = inv(m_b) @ m_a for a = idx_a[p], b = idx_b[p] (poses (n_poses,4,4) f64 row-major, indices DEVICE int32), evaluated
 * as the affine inverse: R_b^-1 = adjugate / determinant, rotation R_b^-1 R_a, translation R_b^-1 (t_a - t_b) with the
 * difference taken FIRST (np.linalg.inv(m_b) @ m_a cancels digits at UTM-sized translations), three-term dot products summed
 * left to right, last row 0 0 0 1.  negate_translation: the translation is negated afterwards (datasets/mulran/utils.py:
 * 122-124); off: misc/poses.py:89.  status (n_pairs) DEVICE int32: a non-zero EGONN_POSE_STATUS_* pair gets the identity. */
int egonn_relative_poses(const double* poses, int64_t n_poses, const int32_t* idx_a, const int32_t* idx_b, int64_t n_pairs,
                         int negate_translation, double* out, int32_t* status, void* stream);
/* Copies clouds pick[0..n_pick) (DEVICE int32) of a bank (bank (n_bank,3) f64, bank_offsets (n_clouds+1) DEVICE int64: the
 * layout egonn_voxel_downsample returns) back to back into out (capacity,3) and writes out_offsets (n_pick+1) DEVICE int64:
 * the src / src_offsets of egonn_icp_pairs.  n_pick <= 4096 (the scan runs in one workgroup).  A pick outside the bank
 * (EGONN_TUPLES_STATUS_BAD_INDEX) or more than `capacity` points (EGONN_TUPLES_STATUS_CAPACITY) is written to *status (DEVICE
 * int32) and leaves ALL offsets zero and nothing copied: the ICP then sees empty clouds (EGONN_ICP_STATUS_EMPTY). */
int egonn_gather_clouds(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds, const int32_t* pick,
                        int n_pick, double* out, int64_t capacity, int64_t* out_offsets, int32_t* status, void* stream);

/* ------------------------------------------------------------------ voxel map (csrc/voxel_map.hip)
 * A resident global voxel map of posed scans.  The map is defined by `voxel` (fp64, finite, > 0), `origin` (3 HOST doubles,
 * finite) and 21 index bits per axis with bias 2^20.  Observation k is the bank cloud pick[k] under the pose X_k ((4,4) fp64
 * row-major, scan frame -> map frame); for a point p of it, per axis a and with every operation rounded to fp64 (no FMA):
 *     t'_a = X_k[a][3] - origin_a                                   (first: poses may carry UTM-sized translations)
 *     w_a  = ((X_k[a][0] p_0 + X_k[a][1] p_1) + X_k[a][2] p_2) + t'_a
 *     s_a  = w_a / voxel;   i_a = floor(s_a);   the point is valid iff every i_a is finite and in [-2^20, 2^20)
 *     key  = (i_x + 2^20) << 42 | (i_y + 2^20) << 21 | (i_z + 2^20)                                    (bit 63 clear)
 *     q_a  = min((int64) floor((s_a - i_a) * 2^30), 2^30 - 1)       (s_a = -1e-20: i_a = -1 and s_a - i_a rounds to 1.0)
 * A voxel record is key (uint64), sum_q[3] (int64: the sums of its points' q), count (int32: points) and obs (int32:
 * observations that put at least one point in it), held as four arrays (keys (rows), sums (rows,3), count (rows), obs
 * (rows): 40 bytes per voxel), sorted by ascending key, keys unique.  Its centroid is
 *     c_a = ((double) i_a + (double) sum_q_a / ((double) count * 2^30)) * voxel + origin_a.
 * The sums are integers: inserting observations in any number of batches and in any order gives the bits of one call, and the
 * kernels reduce a voxel's run in whatever order the hardware takes (integer atomics only; no floating-point atomic).
 * Every call: scratch 256-byte aligned and at least *_scratch_bytes (-1 on bad arguments), no host synchronisation,
 * capturable; grids are sized from the capacities, the live counts (n_out, n_a, n_b, n_dev: DEVICE int64, clipped to their
 * capacity) stay on the device.  *status (DEVICE int32) is OR-ed into, never cleared: the caller zeroes it. */
enum { EGONN_VMAP_STATUS_RANGE = 1,       /* a point was dropped: an index outside 21 bits or a non-finite coordinate */
       EGONN_VMAP_STATUS_CAPACITY = 2,    /* more points / voxels than the capacity: see each call */
       EGONN_VMAP_STATUS_BAD_INDEX = 4 }; /* a pick outside the bank: that observation contributes nothing */
/* The records of observations 0..n_obs) (1 <= n_obs <= 4096): bank (n_bank,3) f64 with bank_offsets (n_clouds+1) DEVICE int64
 * (the layout egonn_voxel_downsample returns), pick (n_obs) DEVICE int32, poses (n_obs,4,4) DEVICE f64.  points_capacity
 * (< 2^31) is a host bound on the picked clouds' total, as egonn_gather_clouds takes `capacity`; more points than that set
 * CAPACITY and give n_out = 0.  out_* hold `capacity` rows; more voxels than that set CAPACITY, n_out = 0 and nothing is
 * written.  A dropped point sets RANGE and every other point is fused as if it were absent.  obs of a voxel counts the distinct
 * positions k among its points: the same cloud picked twice is two observations. */
int64_t egonn_voxel_map_integrate_scratch_bytes(int64_t points_capacity, int n_obs);
int egonn_voxel_map_integrate(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds, const int32_t* pick,
                              const double* poses, int n_obs, const double* origin, double voxel, int64_t points_capacity,
                              uint64_t* out_keys, int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t capacity,
                              int64_t* n_out, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream);
/* out = the union of records A (n_a rows) and B (n_b rows) by key; for a key in both, sum_q, count and obs are added (the
 * caller guarantees disjoint observation sets).  capacity_out >= capacity_a; out is neither A nor B.  A union beyond
 * capacity_out sets CAPACITY, out becomes A unchanged (n_out = n_a) and B is dropped whole. */
int64_t egonn_voxel_map_merge_scratch_bytes(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out);
int egonn_voxel_map_merge(const uint64_t* a_keys, const int64_t* a_sums, const int32_t* a_count, const int32_t* a_obs,
                          const int64_t* n_a, int64_t capacity_a, const uint64_t* b_keys, const int64_t* b_sums,
                          const int32_t* b_count, const int32_t* b_obs, const int64_t* n_b, int64_t capacity_b, uint64_t* out_keys,
                          int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t capacity_out, int64_t* n_out,
                          int32_t* status, void* scratch, int64_t scratch_bytes, void* stream);
/* Centroids of the voxels with count >= min_count and obs >= min_obs, in ascending key order, per box: boxes (n_boxes,6)
 * DEVICE f64 = centre and half extents in the map frame (n_boxes <= 4096; null with n_boxes = 0: the whole map is one
 * segment).  A voxel belongs to box b iff centre_a - half_a <= c_a < centre_a + half_a on every axis.  relative (needs boxes):
 * the output point is c - centre, the local coordinates egonn_icp_pairs wants as tgt.  out_points (capacity,3),
 * out_offsets (max(n_boxes,1)+1) DEVICE int64, out_count / out_obs (capacity) nullable.  More selected voxels than
 * `capacity`: CAPACITY, all offsets zero, nothing written (egonn_gather_clouds' rule).  out_points = null is the sizing call:
 * the offsets are written and nothing else. */
int64_t egonn_voxel_map_select_scratch_bytes(int64_t capacity_map, int n_boxes);
int egonn_voxel_map_select(const uint64_t* keys, const int64_t* sums, const int32_t* count, const int32_t* obs, const int64_t* n_dev,
                           int64_t capacity_map, const double* origin, double voxel, int min_count, int min_obs, const double* boxes,
                           int n_boxes, int relative, double* out_points, int64_t* out_offsets, int32_t* out_count, int32_t* out_obs,
                           int64_t capacity, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ map update (csrc/voxel_map.hip)
 * Records with moments, and taking observations out again.  A map may carry two more arrays per voxel beside keys / sums /
 * count / obs: s1 (rows,3) int64 and s2 (rows,6) int64, exactly the NDT layer's moments below (m_a = q_a >> 10, s1 = sum m,
 * s2 = sum m_a m_b in the order xx, xy, xz, yy, yz, zz) over the points of the voxel; count is that layer's cnt.  In each of
 * the calls of this section the moment arrays of ALL operands (A, B, out) are either all given or all null; a mixed set is
 * refused before the first HIP call.  With all of them null a call is its plain counterpart.  The rules of the voxel-map
 * section hold (scratch, no host synchronisation, capturable, live counts on the device, *status OR-ed into).
 *
 * integrate_moments: keys / sums / count / obs / n_out / status are those of egonn_voxel_map_integrate, bit for bit; s1 / s2
 *   are what egonn_ndt_accumulate gives over those keys for the same observations.  The moments are formed from the q of a
 *   point's row while its run is reduced: no extra per-point storage (the scratch is integrate's), integer atomics only.
 * merge_moments: egonn_voxel_map_merge (positions, the capacity rule out = A with B dropped whole, the bits of the four
 *   arrays) with s1 / s2 added on matched rows and copied on the others.
 * subtract: out = A - B.  For a B row with key k let r = A[k] - B[k], field by field over sums, count, obs, s1, s2 (int64 sums
 *   wrap as the additions did).  The B row is LEGAL iff k is in A and either r.count > 0 and r.obs > 0, or every field of r is
 *   zero.  If every B row is legal, out holds in ascending key order A's rows with r in place of the matched ones, the rows
 *   with r.count == 0 left out, and n_out = n_a - (rows left out).  If any B row is not legal, EGONN_VMAP_STATUS_MISMATCH is
 *   OR-ed into *status and out becomes A unchanged (n_out = n_a, moments included): a map never loses what it holds.
 *   capacity_out >= capacity_a, so CAPACITY is never set; out is neither A nor B; rows from n_out on are not written;
 *   n_b = 0 gives out = A.  B's keys are ascending and unique, as every record set is.
 *   What subtract does NOT prove: that B is what was once added.  An observation re-integrated under a wrong pose that happens
 *   to hit the same voxels with smaller counts passes and leaves wrong sums.  Exactness is the caller's: remove an
 *   observation under the pose (to the bit), the origin and the voxel size it was inserted with (Python keeps a ledger). */
enum { EGONN_VMAP_STATUS_MISMATCH = 8 };  /* subtract: a B row that A does not hold (absent key, or more than A holds): out = A */
int64_t egonn_voxel_map_integrate_moments_scratch_bytes(int64_t points_capacity, int n_obs);
int egonn_voxel_map_integrate_moments(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds,
                                      const int32_t* pick, const double* poses, int n_obs, const double* origin, double voxel,
                                      int64_t points_capacity, uint64_t* out_keys, int64_t* out_sums, int32_t* out_count,
                                      int32_t* out_obs, int64_t* out_s1, int64_t* out_s2, int64_t capacity, int64_t* n_out,
                                      int32_t* status, void* scratch, int64_t scratch_bytes, void* stream);
int64_t egonn_voxel_map_merge_moments_scratch_bytes(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out);
int egonn_voxel_map_merge_moments(const uint64_t* a_keys, const int64_t* a_sums, const int32_t* a_count, const int32_t* a_obs,
                                  const int64_t* a_s1, const int64_t* a_s2, const int64_t* n_a, int64_t capacity_a,
                                  const uint64_t* b_keys, const int64_t* b_sums, const int32_t* b_count, const int32_t* b_obs,
                                  const int64_t* b_s1, const int64_t* b_s2, const int64_t* n_b, int64_t capacity_b,
                                  uint64_t* out_keys, int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t* out_s1,
                                  int64_t* out_s2, int64_t capacity_out, int64_t* n_out, int32_t* status, void* scratch,
                                  int64_t scratch_bytes, void* stream);
int64_t egonn_voxel_map_subtract_scratch_bytes(int64_t capacity_a, int64_t capacity_b, int64_t capacity_out);
int egonn_voxel_map_subtract(const uint64_t* a_keys, const int64_t* a_sums, const int32_t* a_count, const int32_t* a_obs,
                             const int64_t* a_s1, const int64_t* a_s2, const int64_t* n_a, int64_t capacity_a,
                             const uint64_t* b_keys, const int64_t* b_sums, const int32_t* b_count, const int32_t* b_obs,
                             const int64_t* b_s1, const int64_t* b_s2, const int64_t* n_b, int64_t capacity_b, uint64_t* out_keys,
                             int64_t* out_sums, int32_t* out_count, int32_t* out_obs, int64_t* out_s1, int64_t* out_s2,
                             int64_t capacity_out, int64_t* n_out, int32_t* status, void* scratch, int64_t scratch_bytes,
                             void* stream);

/* ------------------------------------------------------------------ NDT layer (csrc/ndt.hip)
 * One Gaussian per voxel over the keys of a voxel map, and the normal-distributions transform against them.  The layer lies
 * over a fixed, ascending, unique key array keys[0 .. n) (n = *n_dev clipped to capacity_map: a snapshot of a map's keys) and
 * uses the map's `voxel` and `origin`.  The point arithmetic is the voxel map's, bit for bit (t', w, s, i, key, q above).
 *
 * Moments.  m_a = q_a >> 10 (20 bits: a voxel holds the squares of 2^23 points in an int64).  Three arrays over the rows:
 *     cnt (rows) int32;   s1 (rows,3) int64 = sum m;   s2 (rows,6) int64 = sum m_a m_b in the order xx, xy, xz, yy, yz, zz.
 * A valid point whose key is in keys adds to its row; one whose key is absent adds 1 to *missed (DEVICE int64); a dropped point
 * sets EGONN_VMAP_STATUS_RANGE, a bad pick BAD_INDEX, more points than points_capacity CAPACITY and then nothing is added (the
 * rules of egonn_voxel_map_integrate).  The call adds into arrays the caller zeroed.  Everything is an integer: any batching
 * and any order of calls give the bits of one call; there is no floating-point atomic.
 *
 * Gaussians.  Every operation rounded to fp64 in the order written (no FMA):
 *     nf = (double) cnt;   mu_a = (double) s1_a / nf;   mean_a = ((double) i_a + mu_a * 2^-20) * voxel    (relative to origin)
 *     u = voxel * 2^-20;   C_ab = ((((double) s2_ab - ((double) s1_a * (double) s1_b) / nf) / (nf - 1.0)) * u) * u
 *     C = V diag(l) V^T by cyclic Jacobi (the schedule of the surface normals), eigenvalues ascending, ties in column order
 *     l'_i = max(l_i, min_eig_ratio * l_2);   info_ab = sum_i ((1 / l'_i) v_ai) v_bi, added in i = 0, 1, 2 from 0.0
 *     normal = v_0, negated when its first non-zero component is negative (a map has no sensor to face)
 *     valid iff cnt >= min_points and l_2 > 0 and every value is finite; an invalid row is all zeros, valid = 0.
 * min_points = 6 and min_eig_ratio = 0.01 are the Python defaults: choices, not tuned values.  mean (rows,3), info (rows,6:
 * xx, xy, xz, yy, yz, zz), eigenvalues (rows,3), normal (rows,3), valid (rows) uint8, *n_valid DEVICE int64 (set, not added to),
 * cov (rows,6) nullable debug output.  Rows from n on are not written.
 *
 * Registration of a pair (a source cloud, T_init in the origin-relative map frame; null = identity).  Under T_k, for a source
 * point p: vs_a = ((R_a0 p_0 + R_a1 p_1) + R_a2 p_2) + t_a, i_a = floor(vs_a / voxel).  Neighbour offsets in this order: (0,0,0),
 * (+1,0,0), (-1,0,0), (0,+1,0), (0,-1,0), (0,0,+1), (0,0,-1); neighbors = 1 takes the first, 7 all.  A neighbour counts iff its
 * index is in [-2^20, 2^20) on every axis, its key is in keys and its row is valid.  Per counted term:
 *     r = vs - mean,  g = info r,  m = r . g,  w = exp(-0.5 m)  (a term with non-finite m is skipped)
 *     n_term += 1,  score += w,  A += w J^T info J (21 upper entries),  b += w J^T g,  J = [-[vs]x | I]: J^T g = (vs x g, g)
 * n_pts = points with at least one term, fitness = n_pts / n_source, the `score` output = score / n_source.
 * Round k: A x = -b by the LDL^T of the point-to-plane ICP (pivot rule 2^-40), U = [Rz(x2) Ry(x1) Rx(x0) | (x3, x4, x5)],
 * T_k+1 = U T_k.  The loop stops, in this order of precedence at the evaluation of T_k: after a round whose step had
 * max |x_0..2| < eps_rot and max |x_3..5| < eps_trans (the new T is evaluated and returned, no bit set); k = max_iteration
 * (MAX_ITER); n_term < 6 (FEW_CORR); a failed pivot or a non-finite step (SINGULAR); T is unchanged by the last three.  A pair
 * without source points: EMPTY, T = T_init.  iterations = steps taken.  This is the Gauss-Newton form of the NDT score: the
 * Hessian sum w J^T info J is positive semi-definite and there is no line search; Magnusson's full Newton step with
 * More-Thuente is not built.  Python's defaults max_iteration = 30, eps_rot = 1e-5, eps_trans = 1e-4 are choices.
 * Summation order: a lane adds its terms in neighbour order, a workgroup of 256 consecutive source points of one pair reduces
 * in a fixed tree, partials are added in ascending workgroup order: a pair has the same bits alone, in any batch, at any
 * position.  Debug tables (nullable): T_trace (n_pairs, max_iteration+1, 4, 4) = T_k (zero beyond the stop), eval_trace
 * (n_pairs, max_iteration+1, 4) = n_term, n_pts, score, stop of the evaluation of T_k, sums_trace (n_pairs, max_iteration+1,
 * 30) = its sums: n_term, n_pts, A (21 upper entries row by row), b (6), score.  status reuses EGONN_ICP_STATUS_*.
 * Every call: arguments are checked before the first HIP call; scratch 256-byte aligned, at least *_scratch_bytes (-1 on bad
 * arguments); 1 <= n_obs, n_pairs <= 4096; sizes in [0, 2^31); no host synchronisation, capturable. */
int64_t egonn_ndt_accumulate_scratch_bytes(int64_t points_capacity, int n_obs);
int egonn_ndt_accumulate(const double* bank, int64_t n_bank, const int64_t* bank_offsets, int64_t n_clouds, const int32_t* pick,
                         const double* poses, int n_obs, const double* origin, double voxel, int64_t points_capacity,
                         const uint64_t* keys, const int64_t* n_dev, int64_t capacity_map, int32_t* cnt, int64_t* s1, int64_t* s2,
                         int64_t* missed, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream);
int egonn_ndt_finalize(const uint64_t* keys, const int64_t* n_dev, int64_t capacity_map, const int32_t* cnt, const int64_t* s1,
                       const int64_t* s2, double voxel, int min_points, double min_eig_ratio, double* mean, double* info,
                       double* eigenvalues, double* normal, uint8_t* valid, int64_t* n_valid, double* cov, void* stream);
int64_t egonn_ndt_register_scratch_bytes(int64_t n_src, int n_pairs);
int egonn_ndt_register(const double* src, int64_t n_src, const int64_t* src_offsets, int n_pairs, const double* T_init,
                       const uint64_t* keys, const int64_t* n_dev, int64_t capacity_map, const double* mean, const double* info,
                       const uint8_t* valid, double voxel, int neighbors, int max_iteration, double eps_rot, double eps_trans,
                       double* T, double* fitness, double* score, int32_t* iterations, int32_t* status, double* T_trace,
                       double* eval_trace, double* sums_trace, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ relocalisation against a keypoint map (csrc/relocalize.hip, csrc/match.hip)
 * A query scan is placed in the map frame by registering it against its top-k retrieved map entries (egonn_knn) and keeping
 * the entry with the most inliers: P_query = P_map[best] @ T, T = the transform of egonn_registration_finish, which maps query
 * keypoints into the candidate's frame (misc/poses.py: T_gt = inv(P_map) @ P_query).  The map is resident: descriptors
 * bank_feat (n_bank, n_max, dim) f32, keypoints bank_kp (n_bank, n_max, 3) f32, counts bank_n (n_bank) int32, poses
 * map_pose (n_bank,4,4) f64.  Queries: q_feat (n_queries, n_max, dim), q_kp, q_n; nn_index (n_queries, k) DEVICE int32 map
 * entries per query, -1 = none (what egonn_knn writes beyond the map).  Pair p = q * k + c.  1 <= k <= 1024, n_queries * k <=
 * 2^20, n_bank >= 1, n_max <= 256.  The sequence egonn_match_candidates, egonn_gather_candidates, egonn_ransac_pairs,
 * egonn_registration_finish, egonn_pick_candidates has no host synchronisation and can be captured. */
enum { EGONN_RELOC_NO_CANDIDATE = 1,     /* candidate index -1 (or outside the map): an empty pair */
       EGONN_RELOC_BAD_INDEX = 2,        /* candidate index < -1 or >= n_bank: an empty pair, nothing read */
       EGONN_RELOC_UNVERIFIED = 4 };     /* per query: no candidate with a model and min_inliers inliers */
/* bytes of the scratch of egonn_match_candidates (-1 on bad arguments) */
int64_t egonn_match_candidates_scratch_bytes(int n_queries, int k, int n_max);
/* the indexed addressing of the matching operator (see egonn_match_mutual; csrc/match.hip): pair p = q * k + c matches
 * query q against bank entry nn_index[q][c], read by index: nothing is gathered, and the result has the bits
 * egonn_match_mutual gives on gathered operands (counts clipped to [0, n_max]).  dim a multiple of 4 up to 256, descriptors
 * 16-byte aligned, scratch 8-byte aligned.  corr (n_queries * k, n_max, 2) int32, n_corr (n_queries * k), status
 * (n_queries * k) int32 of EGONN_RELOC_* bits (nullable).  An invalid index gives n_corr = 0 and all rows -1; nothing is
 * read by it. */
int egonn_match_candidates(const float* q_feat, const int32_t* q_n, const float* bank_feat, const int32_t* bank_n,
                           const int32_t* nn_index, int n_queries, int k, int n_bank, int n_max, int dim, int32_t* corr,
                           int32_t* n_corr, int32_t* status, void* scratch, int64_t scratch_bytes, void* stream);
/* the keypoint operands of egonn_ransac_pairs / egonn_registration_finish for the same pairs: kp1 (P, n_max, 3) = the
 * query's keypoints repeated, kp2 = the candidate's (zeros for an invalid index), n1 = q_n[q], n2 = bank_n[index] (0 for an
 * invalid index), pair_id = (query_id[q] * 1000003 + index) mod 2^30 with query_id (n_queries) DEVICE int32, null = q: a
 * pair's draws depend on the query's id and the map entry, not on the candidate's rank nor on the batch. */
int egonn_gather_candidates(const float* q_kp, const int32_t* q_n, const float* bank_kp, const int32_t* bank_n,
                            const int32_t* nn_index, const int32_t* query_id, int n_queries, int k, int n_bank, int n_max,
                            float* kp1, float* kp2, int32_t* n1, int32_t* n2, int32_t* pair_id, void* stream);
/* per query over the k results of egonn_registration_finish (T (P,4,4) f64, inliers, inlier_rmse, reg_status (P); rte, rre,
 * success (P) nullable): candidates ordered by most inliers, then lowest inlier_rmse, then lowest rank; invalid candidates
 * last in rank order.  reranked (n_queries, k) = the map indices in that order (-1 for invalid ones).  The head of the order
 * wins if it is valid, has a model (no EGONN_REG_STATUS_NO_MODEL) and inliers >= min_inliers: best_rank, best_index, best_inliers
 * (n_queries), T_rel (n_queries,4,4) = its T, pose = map_pose[best] @ T_rel as the affine product (three-term dot products
 * summed left to right, then the translation added; last row 0 0 0 1), best_rte / best_rre / best_success (nullable) = its
 * metrics.  Otherwise EGONN_RELOC_UNVERIFIED: best_rank = best_index = -1, best_inliers = 0, T_rel = pose = identity, best_rte =
 * best_rre = -1, best_success = 0.  safe_pick (n_queries) = best_index when verified, else nn_index[q][0] clamped to
 * [0, n_bank): a pick egonn_gather_clouds accepts.  status (n_queries) = OR of the candidates' EGONN_RELOC_* bits. */
int egonn_pick_candidates(const int32_t* nn_index, int n_queries, int k, int n_bank, const double* map_pose, const double* T,
                          const int32_t* inliers, const double* inlier_rmse, const int32_t* reg_status, const double* rte,
                          const double* rre, const int32_t* success, int min_inliers, int32_t* best_rank, int32_t* best_index,
                          int32_t* reranked, double* T_rel, double* pose, int32_t* safe_pick, int32_t* best_inliers,
                          int32_t* status, double* best_rte, double* best_rre, int32_t* best_success, void* stream);

/* ------------------------------------------------------------------ loop closure inside one trajectory (csrc/loop_closure.hip)
 * "Has the vehicle been here before?": every scan of a growing trajectory is searched against the scans that are old enough.
 * Every entry point validates its arguments before any launch (EGONN_STATUS_INVALID), takes a stream and never synchronises.
 *
 * egonn_time_windows: the admissible window [win_lo[q], win_hi[q]) of every query from float64 time stamps (Unix-time stamps
 * at 0.1 s spacing do not survive fp32), one binary search per bound: win_hi[q] = #{j : t_db[j] <= t_q[q] - min_gap} (the bound
 * is inclusive), win_lo[q] = #{j : t_db[j] < t_q[q] - max_gap} (max_gap = +inf: 0).  t_db (m) must be non-decreasing; status
 * (DEVICE, 1 int) bit 0 is set when it is not (a NaN stamp counts), the windows are then unspecified but inside [0, m].
 *
 * egonn_knn_window: egonn_knn of query q on database[lo:hi], lo = max(win_lo[q], 0) (win_lo NULL = 0), hi = min(win_hi[q],
 * n_database), with lo added to the indices: ascending distance, ties to the lower index, (-1, +inf) where fewer than k rows are
 * admissible (lo >= hi: the whole list), the +inf / NaN rules of egonn_knn, and distances bit-identical to egonn_knn's (the two
 * kernels share the row-distance function).  win_lo / win_hi: DEVICE (n_query) int32.  1 <= k <= 64, 1 <= dim <= 4096,
 * n_database >= 0 (0: every list is empty), n_query = 0 returns at once.  There is no n_query x n_database buffer: the k best
 * are kept while the rows stream past, and the result of a query does not depend on the other queries of the call.  The
 * scratch (8-byte aligned, 0 bytes for 512 queries or more: NULL is accepted then) depends on n_query and k only.
 *
 * egonn_window_radius: count[q] = rows j of the window with sqrtf(sum_c fmaf(d_c, d_c, .)) <= radius, d_c = qpos[q][c] -
 * dbpos[j][c] (the form and component order of egonn_recall_counts; position_dim 2 or 3); with pred (n_query, nullable):
 * pred_dist[q] = that distance to row pred[q], +inf when pred[q] < 0 or >= m.
 *
 * egonn_pr_curve: the precision/recall curve of n decisions.  A lower score is more confident; +inf or NaN = no prediction;
 * -0.0 counts as +0.0; negative scores are legal.  order (n) = the stable ascending order by (score, index), predictions first
 * (the flat radix sort on the monotone map of the float's bits); cum_tp / cum_fp / cum_rev (n) = inclusive counts over
 * positions 0..i of correct != 0 / correct == 0 / revisit != 0 among the predictions (positions behind the last prediction
 * repeat its counts); group_end[i] = 1 where position i is the last of a run of equal scores among the predictions: the points
 * of the curve; totals (DEVICE, 2) = number of predictions, number of revisit != 0 over all n.  scratch: 256-byte aligned. */
int egonn_time_windows(const double* t_db, int64_t m, const double* t_q, int64_t n_query, double min_gap, double max_gap,
                       int32_t* win_lo, int32_t* win_hi, int32_t* status, void* stream);
int64_t egonn_knn_window_scratch_bytes(int64_t n_query, int k);      /* -1 on bad arguments; no dependence on n_database */
int egonn_knn_window(const float* query, int64_t n_query, const float* database, int64_t n_database, int dim, int k,
                     const int32_t* win_lo, const int32_t* win_hi, int32_t* out_index, float* out_distance, void* scratch,
                     int64_t scratch_bytes, void* stream);
int egonn_window_radius(const float* query_positions, int64_t n_query, const float* db_positions, int64_t m, int position_dim,
                        const int32_t* win_lo, const int32_t* win_hi, float radius, const int32_t* pred, int32_t* count,
                        float* pred_dist, void* stream);
int64_t egonn_pr_curve_scratch_bytes(int64_t n);                      /* -1 on bad arguments */
int egonn_pr_curve(const float* score, const int32_t* correct, const int32_t* revisit, int64_t n, int32_t* order,
                   int32_t* cum_tp, int32_t* cum_fp, int32_t* cum_rev, uint8_t* group_end, int32_t* totals, void* scratch,
                   int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ pose-graph optimisation (csrc/pose_graph.hip)
 * The corrected trajectory behind the loop detector.  Unknowns: poses X_i = [R_i | t_i] as (n,4,4) float64; edge e = (a, b, Z,
 * (w_rot, w_trans)) measures Z ~ X_a^-1 X_b, weights in 1/sigma^2, both 0 = off.  E = Z^-1 X_a^-1 X_b, r = [t_E ; Log_SO3 R_E],
 * s = sqrt(w_trans |t_E|^2 + w_rot |Log R_E|^2), rho = 1 or, robust_delta > 0, min(1, delta / s) (Huber by IRLS: recomputed at
 * every linearisation, fixed inside the linear solve), cost = sum rho (1 - rho / 2) s^2 (s^2 / 2, and delta s - delta^2 / 2 beyond
 * delta: the Huber cost, whose gradient is sum J^T rho W r).  Retraction R <- R Exp(w), t <- t + R v for
 * delta_i = (v, w), followed by one Newton-Schulz step on R; a node whose delta is exactly 0 is copied bit for bit.  Residual
 * rotations up to pi - 1e-3; beyond, EGONN_PG_STATUS_ANGLE and weight 0 for that linearisation.
 * Every entry point validates its arguments before any launch (EGONN_STATUS_INVALID), takes a stream, never synchronises and is
 * deterministic (no floating-point atomics; sums in one fixed order).  All pointers are DEVICE pointers.  scratch: one span of
 * egonn_pose_graph_scratch_bytes(n, E, pcg_iterations) bytes, 256-byte aligned, owned by the caller; egonn_pose_graph_plan
 * fills its plan part and the other three calls need that plan of the same (n, E) in the same span.
 *
 * egonn_pose_graph_plan: validates the edges and builds the node -> (edge, side) lists, each in edge order.  edge_index (E,2)
 * int32, Z (E,4,4), weights (E,2) or NULL (all 1), fixed (n) uint8 or NULL (node 0 only).  edge_status (E): BAD_INDEX (outside
 * [0, n)), SELF_LOOP, NONFINITE (a non-finite entry of Z or the weights, or a last row of Z other than 0 0 0 1),
 * NEGATIVE_WEIGHT; an edge with a bit set is off.  graph_status (1): ISOLATED when a free node has no live edge.
 * egonn_pose_graph_cost: cost (1), residuals (E,6) = [t_E ; Log R_E], rho (E), s (E), gradient (n,6) = sum J^T W r in (v, w)
 * order for EVERY node (the gauge is the solver's), edge_status (E) = the plan's bits | ANGLE.  An edge that is off (by the plan
 * or by ANGLE) gives residual 0, s 0, rho 1.  Poses are not validated up front: an edge whose residual is not finite (a
 * non-finite pose) is switched off with the ANGLE bit as well.
 * egonn_pose_graph_odometry: the chain of a trajectory, edge_index (n-1,2) = (i, i + 1), Z (n-1,4,4) = X_i^-1 X_{i+1}.
 * egonn_pose_graph_hessvec: out (n,6) = (J^T W J + lambda I) p on the free nodes, the product the solver iterates with: rows of
 * fixed nodes are 0 and their p is ignored.
 * egonn_pose_graph_optimize: max_iterations Levenberg-Marquardt steps, each a linearisation, exactly pcg_iterations iterations of
 * block-Jacobi preconditioned conjugate gradients (two launches each; after |r| <= pcg_tol |r0| in the M^-1 norm or p.Hp <= 0
 * they return at once) on (J^T W J + lambda I) delta = -J^T W r, the retraction into a candidate and its cost.  Accepted when the
 * cost decreases (lambda <- max(lambda / 10, lambda_min)), otherwise the poses stay and lambda <- 10 lambda.  Stops (every later
 * launch returns at once) on a relative decrease < rel_tol, lambda > lambda_max or a gradient max-norm <= grad_tol.  poses_out
 * (n,4,4); cost_trace (max_iterations + 1): the cost of the start and after every step, NaN after the stop; accept_trace
 * (max_iterations): 1 / 0 / -1 (not run); counters (2) = steps run, steps accepted; lambda_out (1); edge_status (E) = the plan's
 * bits | ANGLE of any linearisation; graph_status (1) = the plan's | PIVOT (a diagonal block fell back to the identity). */
enum {
  EGONN_PG_STATUS_BAD_INDEX = 1,
  EGONN_PG_STATUS_SELF_LOOP = 2,
  EGONN_PG_STATUS_NONFINITE = 4,
  EGONN_PG_STATUS_NEGATIVE_WEIGHT = 8,
  EGONN_PG_STATUS_ANGLE = 16,
  EGONN_PG_STATUS_ISOLATED = 32,
  EGONN_PG_STATUS_PIVOT = 64
};
int64_t egonn_pose_graph_scratch_bytes(int64_t n, int64_t n_edges, int pcg_iterations);     /* -1 on bad arguments */
int egonn_pose_graph_odometry(const double* poses, int64_t n, double* Z, int32_t* edge_index, void* stream);
int egonn_pose_graph_plan(const int32_t* edge_index, const double* Z, const double* weights, const uint8_t* fixed, int64_t n,
                          int64_t n_edges, int32_t* edge_status, int32_t* graph_status, void* scratch, int64_t scratch_bytes,
                          void* stream);
int egonn_pose_graph_cost(const double* poses, int64_t n, int64_t n_edges, const double* Z, double robust_delta, double* cost,
                          double* residuals, double* rho, double* s, double* gradient, int32_t* edge_status, void* scratch,
                          int64_t scratch_bytes, void* stream);
int egonn_pose_graph_hessvec(const double* poses, int64_t n, int64_t n_edges, const double* Z, double robust_delta, double lambda,
                             const double* p, double* out, int32_t* edge_status, void* scratch, int64_t scratch_bytes,
                             void* stream);
int egonn_pose_graph_optimize(const double* poses, int64_t n, int64_t n_edges, const double* Z, double robust_delta,
                              int max_iterations, int pcg_iterations, double pcg_tol, double lambda_init, double lambda_min,
                              double lambda_max, double rel_tol, double grad_tol, double* poses_out, double* cost_trace,
                              int32_t* accept_trace, int32_t* counters, double* lambda_out, int32_t* edge_status,
                              int32_t* graph_status, void* scratch, int64_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------ loop-edge consistency filter (csrc/loop_consistency.hip)
 * Between the loop edges and the pose graph: two loop closures taken close together in time must agree with each other through
 * the odometry between them.  poses (n,4,4) float64, the drifting trajectory; edge_index (E,2) int32 = (a, b), Z (E,4,4) ~
 * X_a^-1 X_b, weights (E,2), E static.  An edge is live when the pose-graph plan would leave it on (no BAD_INDEX, SELF_LOOP,
 * NONFINITE, NEGATIVE_WEIGHT; a non-finite pose at either end also gives NONFINITE) and one of its weights is positive; a dead
 * edge never votes, has support 0, keep 0, and leaves every other output bit-equal to a call without it.
 * Cycle of live edges e, f: C = Z_e (X_be^-1 X_bf) Z_f^-1 (X_af^-1 X_ae), c_trans = |t_C|, c_rot = |Log_SO3 R_C|, always with the
 * edge that comes first in the order of (b, row) in the role of e, so the relation is symmetric by construction.
 * Comparable: |b_e - b_f| <= window, |a_e - a_f| <= window, and at most max_partners / 2 positions apart in the order of the live
 * edges by (b, row); TRUNCATED when a live edge has a partner inside its b-window beyond that cap.  Consistent: comparable,
 * c_trans <= trans_thr + trans_drift g, c_rot <= rot_thr + rot_drift g, g = |b_e - b_f| + |a_e - a_f|.  An edge never counts
 * itself; duplicates count each other.  Selection: the min_support-core in synchronous rounds (count, then remove all below
 * min_support at once); max_rounds rounds are enqueued, after one that removed nothing the rest return at once; ROUNDS when
 * the last round still removed something.  Not a maximum clique: a coherent set of false loops survives.
 * Outputs: keep (E) uint8, support0 (E) before any removal, support (E) among the survivors (0 for removed and dead edges),
 * weights_out (E,2) = weights * keep, rounds (1) = rounds that removed something, edge_status (E) = EGONN_PG_STATUS_* bits,
 * status (1) = EGONN_LC_STATUS_*.  scratch: egonn_loop_consistency_scratch_bytes(E, max_partners) bytes, 256-byte aligned
 * (-1 for E outside [0, 2^30) or max_partners not a multiple of 64 in [64, 65536]).  Arguments are validated before any launch
 * (null or misaligned pointers, n or E out of the plan's ranges, window < 0, thresholds negative or not finite, min_support < 1,
 * max_rounds outside [1, 65536], max_partners, scratch); one stream, no synchronisation, deterministic, float64.
 * egonn_loop_cycle_errors: the test seam of the arithmetic.  pairs (P,2) int32 rows of the edge arrays -> out (P,2) =
 * (c_trans, c_rot) in the canonical role; a pair out of range or naming an edge with a status bit gives NaN (no weights here). */
enum {
  EGONN_LC_STATUS_TRUNCATED = 1,
  EGONN_LC_STATUS_ROUNDS = 2
};
int64_t egonn_loop_consistency_scratch_bytes(int64_t n_edges, int max_partners);            /* -1 on bad arguments */
int egonn_loop_consistency(const double* poses, int64_t n, const int32_t* edge_index, const double* Z, const double* weights,
                           int64_t n_edges, int window, double trans_thr, double rot_thr, double trans_drift, double rot_drift,
                           int min_support, int max_rounds, int max_partners, uint8_t* keep, int32_t* support0, int32_t* support,
                           double* weights_out, int32_t* rounds, int32_t* edge_status, int32_t* status, void* scratch,
                           int64_t scratch_bytes, void* stream);
int egonn_loop_cycle_errors(const double* poses, int64_t n, const int32_t* edge_index, const double* Z, int64_t n_edges,
                            const int32_t* pairs, int64_t n_pairs, double* out, void* stream);

/* ------------------------------------------------------------------ launch timing (bench.py roofline leg)
 * mode 0: off; 1: time every tagged sparse-conv launch (event records around it); 2: only launches whose tag contains
 * `filter`, with the events attached to the kernel dispatch itself (the kernel's own begin..end, also when other streams
 * share the GPU); 3: like 2 but as event-record brackets, which a stream capture turns into graph nodes — the records of
 * a captured sequence are re-recorded by every replay and egonn_profile_fetch returns the LAST replay's durations. */
int egonn_profile_enable(egonn_ctx* ctx, int mode, const char* filter);
/* Drain the records collected since the last fetch.  [SYNC]  names: cap x 64 chars.  bytes = the algorithmic
 * bytes of SURVEY.md §8(d) (P*Cin*4 + N_out*Cout*4 + K*Cin*Cout*4 + 8*P), flops = 2*P*Cin*Cout. */
int egonn_profile_fetch(egonn_ctx* ctx, int cap, int* n, char* names, float* ms, double* bytes, double* flops,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EGONN_HIP_H */
