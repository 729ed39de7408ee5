/*
 * libmtlssl_hip.so — C ABI of the MI355X (gfx950) hot path for the mtl-ssl
 * Faster R-CNN / R-FCN multi-task detector.
 *
 * Boundary rules:
 *   - plain `extern "C"`; raw DEVICE pointers + integer dims + a hipStream_t passed as void*;
 *   - every function is asynchronous on the given stream and returns 0 on success or a
 *     negative MTLSSL_E* code (message via mtlssl_last_error(), thread-local);
 *   - no ownership transfer: the caller owns every buffer including workspaces;
 *   - all floats are fp32, all indices int32, all images/feature maps NHWC, all boxes
 *     [ymin, xmin, ymax, xmax].
 *
 * Each entry point names the reference (TensorFlow-graph) code it replaces; paths are
 * relative to the reference tree (object_detection/... or slim/...).
 */
#ifndef MTLSSL_HIP_H_
#define MTLSSL_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mtlssl_stream_t; /* hipStream_t */

#define MTLSSL_OK 0
#define MTLSSL_EINVAL (-1)   /* bad argument / unsupported shape */
#define MTLSSL_ELAUNCH (-2)  /* HIP launch error */
#define MTLSSL_ECOMM (-3)    /* RCCL unavailable or an RCCL call failed */

/* Bumped whenever a prototype below changes; mtlssl_abi_version() of the loaded library must equal it (the ctypes
 * loader checks: an older build called through a newer header would receive shifted arguments). */
#define MTLSSL_ABI_VERSION 23

const char* mtlssl_last_error(void);
int mtlssl_abi_version(void);

/* y[i] = e^x[i] in float64 by the fixed IEEE operation sequence of csrc/portable_math.h — the exponential behind
 * every float that decides index work (RPN foreground softmax faster_rcnn_meta_arch.py:1103-1104, the box decoder
 * box_coders/faster_rcnn_box_coder.py:107-108, the score converters builders/post_processing_builder.py:85-123).
 * Exported so that tests can check it bit for bit against oracle/portable_math.py. */
int mtlssl_exp_rn(const double* x, double* y, int64_t n, mtlssl_stream_t stream);

/* ------------------------------------------------------------------ convolution family
 * Replaces slim.conv2d / resnet_utils.conv2d_same (slim/nets/resnet_utils.py:77-122,
 * slim/nets/resnet_v1.py:107-119) + frozen slim.batch_norm + ReLU, and their TF gradient
 * kernels. Implicit GEMM on v_mfma_f32_32x32x2_f32. Filter layout HWIO [R,S,C,K] (TF).
 * Padding is explicit (pad_t/pad_l); out-of-range taps read zero, so TF 'SAME' asymmetry
 * and conv2d_same's explicit padding are both expressed by the caller's pad/OH/OW choice.
 */
typedef struct {
  int32_t N, H, W, C;        /* input  [N,H,W,C]   */
  int32_t K, R, S;           /* filter [R,S,C,K]   */
  int32_t OH, OW;            /* output [N,OH,OW,K] */
  int32_t stride, dilation;
  int32_t pad_t, pad_l;
  int32_t ldy;               /* row stride (floats) of the OUTPUT-side tensor: y of the forward, dy of dgrad / wgrad.
                              * 0 (or K): dense [N,OH,OW,K]. > K: the tensor is the channel slice [c0, c0+K) of a wider
                              * NHWC map with ldy channels and the y / dy pointer already points at channel c0 — this is
                              * tf.concat(axis=3) folded into its producers and the consumers of its gradient
                              * (slim/nets/inception_resnet_v2.py:46,67,88,185-186,213,253: every branch writes its slice
                              * of the concatenated map; the backward reads its slice of the map's gradient in place).
                              * ldy % 4 == 0 and a 16-byte aligned pointer are required; residual / mask / dx stay dense. */
} mtlssl_conv_desc;

/* Epilogue flags. Whatever the flags' values, they are applied in one order (mtl_ssl_amd/csrc/epilogue.h) — forward:
 * + bias, + residual, then one of ReLU / ReLU6 / tanh; input gradient: + residual, + previous contents (ACCUM), then
 * the ReLU or ReLU6 mask. */
#define MTLSSL_EPI_BIAS 1      /* + bias[k] (folded BN shift or conv bias)                  */
#define MTLSSL_EPI_RESIDUAL 2  /* + residual[n,oh,ow,k]                                     */
#define MTLSSL_EPI_RELU 4      /* max(.,0)                                                  */
#define MTLSSL_EPI_TANH 8      /* tanh(.)  (core/mask_predictor.py:105-119)                 */
#define MTLSSL_EPI_RELU6 16    /* min(max(.,0),6) (slim/nets/mobilenet_v1.py)               */
#define MTLSSL_EPI_MASK 32     /* dgrad only: out *= (mask_ref > 0)  (ReLU backward)         */
#define MTLSSL_EPI_ACCUM 64    /* dgrad only: out += existing contents of the output buffer */
#define MTLSSL_EPI_MASK6 128   /* dgrad only: out *= (0 < mask_ref < 6)  (ReLU6 backward)    */

/* Scratch needed by a call in the given mode (0 fwd, 1 dgrad, 2 wgrad); fwd/dgrad use it for
 * split-K partials when the tile grid alone would not fill the 256 CUs (0 when not split).
 * A null workspace is allowed for fwd/dgrad and disables everything that lives in one: Winograd, the input-parity
 * dgrad, the zero-padded pointwise and space-to-depth forms (their problems run on the direct engine or a VALU
 * fallback kernel instead), and the K split and K-split tail of a direct plan (an unsplit tile plan runs). */
int64_t mtlssl_conv2d_workspace_bytes(const mtlssl_conv_desc* d, int mode);
/* y = epilogue(conv(x, w)). */
int mtlssl_conv2d_fwd(const mtlssl_conv_desc* d, const float* x, const float* w,
                      const float* bias, const float* residual, float* y, int epilogue,
                      void* workspace, mtlssl_stream_t stream);
/* dx = conv_transpose(dy, w); epilogue flags MASK (mask_ref, same shape as dx) / ACCUM /
 * RESIDUAL (adds `residual`, same shape as dx, before the mask). */
int mtlssl_conv2d_dgrad(const mtlssl_conv_desc* d, const float* dy, const float* w,
                        const float* residual, const float* mask_ref, float* dx, int epilogue,
                        void* workspace, mtlssl_stream_t stream);
/* Transformed-filter cache of the Winograd layers (3x3 / stride 1, see mtlssl_conv2d_tile_config): the filter
 * transform U = G g G^T depends on the weights only, which change once per optimizer step, while a layer is
 * convolved several times per step (forward, the refiner's second forward, dgrad). A caller may keep U:
 *   bytes   = mtlssl_conv2d_filter_xf_bytes(d, mode)      0 when the planned algorithm of (d, mode) is direct
 *   variant = mtlssl_conv2d_filter_xf_variant(d, mode)    the Winograd variant planned (0 F(4x4,3x3), 1 whole-7-span), -1 direct;
 *                                                         mode 0 / 1 / 2 (the wgrad plan has no filter to cache: see input_xf below)
 *   mtlssl_conv2d_transform_filter(d, mode, variant, w, filter_xf, stream)   mode 0 forward form, 1 dgrad (flipped) form
 * and hand it to the _xf entry points below together with the variant it was made for; a cache made for another
 * variant than the call's plan (or a null one) is ignored and the call transforms the filter itself.
 * mtlssl_conv2d_fwd / _dgrad are the _xf forms without a cache. */
int64_t mtlssl_conv2d_filter_xf_bytes(const mtlssl_conv_desc* d, int mode);
int mtlssl_conv2d_filter_xf_variant(const mtlssl_conv_desc* d, int mode);
int mtlssl_conv2d_transform_filter(const mtlssl_conv_desc* d, int mode, int variant, const float* w, float* filter_xf,
                                   mtlssl_stream_t stream);
/* The same for n filters of one variant in ONE launch, from device tables: w_ptrs / xf_ptrs (n device pointers
 * each), ck (n x int64: C*K of each filter), flip (n x int32: 1 = dgrad form); max_ck = largest C*K. */
int mtlssl_conv2d_transform_filters(int variant, int n, const void* w_ptrs, const void* xf_ptrs, const int64_t* ck,
                                    const int32_t* flip, int64_t max_ck, mtlssl_stream_t stream);
int mtlssl_conv2d_fwd_xf(const mtlssl_conv_desc* d, const float* x, const float* w, const float* bias,
                         const float* residual, float* y, int epilogue, void* workspace, const float* filter_xf,
                         int xf_variant, mtlssl_stream_t stream);
int mtlssl_conv2d_dgrad_xf(const mtlssl_conv_desc* d, const float* dy, const float* w, const float* residual,
                           const float* mask_ref, float* dx, int epilogue, void* workspace, const float* filter_xf,
                           int xf_variant, mtlssl_stream_t stream);
/* Transformed-input reuse within a training step: the Winograd forward and the Winograd filter gradient of one layer
 * both start from V = B^T x B of the same activation x (slim.conv2d's forward and its Conv2DBackpropFilter see the
 * same input tensor). A caller that keeps activations for backward may keep V as well:
 *   variant = mtlssl_conv2d_filter_xf_variant(d, 0), and the same value from (d, 2), else there is nothing to share
 *   bytes   = mtlssl_conv2d_input_xf_bytes(d, variant)
 *   mtlssl_conv2d_fwd_keep(... input_xf, variant ...)   writes V there instead of into the workspace
 *   mtlssl_conv2d_wgrad_xf(... input_xf, variant ...)   skips its own input transform
 * As with the filter cache, a buffer made for another variant than the call's plan is ignored. */
int64_t mtlssl_conv2d_input_xf_bytes(const mtlssl_conv_desc* d, int variant);
int mtlssl_conv2d_fwd_keep(const mtlssl_conv_desc* d, const float* x, const float* w, const float* bias,
                           const float* residual, float* y, int epilogue, void* workspace, const float* filter_xf,
                           int xf_variant, float* input_xf, int input_variant, mtlssl_stream_t stream);
int mtlssl_conv2d_wgrad_xf(const mtlssl_conv_desc* d, const float* x, const float* dy,
                           const float* out_scale, float* dw, float* dbias, float beta,
                           void* workspace, const float* input_xf, int input_variant, mtlssl_stream_t stream);
/* n pointwise (1x1, stride 1) forward convolutions that read the SAME input x in ONE launch (blockIdx.y = problem): the
 * branch-first 1x1 layers of an Inception-ResNet block (slim/nets/inception_resnet_v2.py:36-44, 57-65, 78-86, 165-184,
 * 226-248 — Branch_0 / Branch_1 / Branch_2 `Conv2d_0a_1x1` all take `net`), or conv1 + shortcut of a ResNet unit
 * (slim/nets/resnet_v1.py:102-112). Each problem keeps its own filter [1,1,C,K_i], bias, output pointer, output row
 * stride (ldy_i: 0 = dense, else the channel count of the concatenated map it writes a slice of) and epilogue flags
 * (BIAS / RELU / RELU6 / TANH; no residual); they share N, H, W, C of `d` (d->K is ignored). `entries` is a HOST array
 * of n <= MTLSSL_CONV_GROUP_MAX records (they travel as kernel arguments: no device table, no copy); max_k / sum_k =
 * largest / summed K_i (the library picks the tile for the summed problem and sizes the grid for the widest one). Requirements: C % 16 == 0, every K_i % 4 == 0 and >= 16, 16-byte aligned pointers. Results
 * are those of n mtlssl_conv2d_fwd calls without a K split. */
#define MTLSSL_CONV_GROUP_MAX 4
typedef struct {
  const float* w;            /* [1,1,C,K] */
  float* y;                  /* [N,H,W,K] with row stride ldy (or K) */
  const float* bias;         /* [K] or NULL */
  int32_t K, ldy, epilogue, reserved;
} mtlssl_conv_group_entry;
int mtlssl_conv2d_fwd_grouped(const mtlssl_conv_desc* d, const float* x, int n, const mtlssl_conv_group_entry* entries,
                              int max_k, int sum_k, mtlssl_stream_t stream);
/* Input gradient of n pointwise (1x1, stride 1) convolutions that read the SAME input, in ONE launch and ONE accumulator
 * pass: dx = sum_i dy_i . w_i^T (+ residual, masked) — the branch-first 1x1 layers of an Inception-ResNet block
 * (slim/nets/inception_resnet_v2.py:36-44, 57-65, 78-86: Branch_0 / Branch_1 / Branch_2 `Conv2d_0a_1x1` all take `net`, so
 * tf.gradients adds their input gradients), or conv1 + shortcut of a ResNet unit (slim/nets/resnet_v1.py:102-112). The
 * reduction walks the segments in the order given: segment i brings its own dy [N,H,W,K_i] (row stride ldy_i: 0 = dense,
 * else the channel count of the concatenated map's gradient it is a slice of) and filter [1,1,C,K_i]; they share N, H, W, C
 * of `d` (d->K, d->ldy ignored). `entries` is a HOST array of n <= MTLSSL_CONV_GROUP_MAX records (kernel arguments: no device
 * table). epilogue: RESIDUAL / MASK / MASK6 as in mtlssl_conv2d_dgrad (no ACCUM). Requirements: C % 4 == 0, C >= 16, every
 * K_i % 16 == 0, 16-byte aligned pointers. Equal to n mtlssl_conv2d_dgrad calls chained with ACCUM up to the order of the
 * fp32 sum (one accumulator over sum K_i instead of n rounded partial results). */
typedef struct {
  const float* dy;           /* [N,H,W,K] with row stride ldy (or K) */
  const float* w;            /* [1,1,C,K] */
  int32_t K, ldy;
} mtlssl_conv_seg_entry;
int mtlssl_conv2d_dgrad_segmented(const mtlssl_conv_desc* d, int n, const mtlssl_conv_seg_entry* entries,
                                  const float* residual, const float* mask_ref, float* dx, int epilogue,
                                  mtlssl_stream_t stream);
/* The same with the bias gradient scaled per output channel too: dbias[k] = beta*dbias[k] + dbias_scale[k] * sum dy[:,k]
 * (dbias_scale nullable = 1): a bias that reaches the layer through a folded per-channel factor — the residual scale of
 * the Inception-ResNet blocks, net += scale * (conv(mixed) + b), slim/nets/inception_resnet_v2.py:47-52. */
int mtlssl_conv2d_wgrad_ex(const mtlssl_conv_desc* d, const float* x, const float* dy,
                           const float* out_scale, float* dw, float* dbias, const float* dbias_scale, float beta,
                           void* workspace, const float* input_xf, int input_variant, mtlssl_stream_t stream);
/* dw[r,s,c,k] (beta=0: overwrite, beta=1: accumulate) = sum_pixels x*dy, optionally scaled
 * per output channel by out_scale[k] (frozen-BN fold) and dbias[k] = sum dy (nullable).
 * workspace: mtlssl_conv2d_wgrad_workspace_bytes(d) bytes. */
int64_t mtlssl_conv2d_wgrad_workspace_bytes(const mtlssl_conv_desc* d);
/* Which kernel instantiation a call will use: mode 0 fwd / 1 dgrad / 2 wgrad ->
 * 0: k_conv_mfma<128,128,mode>, 1: <128,64,mode>, 2: <64,64,mode>, 3: <256,128,mode> (8 wavefronts),
 * -1: direct (non-MFMA) path; 4..7: Winograd F(4x4,3x3) (3x3 / stride 1 / SAME layers) with the GEMM stack
 * on tile 0..3; 8..11: the whole-7-span Winograd variant (maps of 7k x 7k) with the GEMM stack on tile 0..3.
 * For profiling attribution only. */
int mtlssl_conv2d_tile_config(const mtlssl_conv_desc* d, int mode);
/* Autotuning hook: pin the algorithm + tile configuration (0: 128x128, 1: 128x64, 2: 64x64, 3: 256x128
 * direct implicit GEMM; 4..7 / 8..11: Winograd F(4x4,3x3) / whole-7-span with that GEMM tile, ignored for
 * problems outside its domain; < 0 clears) the planner uses for this problem and mode; the K split / tail split is still
 * planned for that tile. The caller times the candidates on its own tensors (mtl_ssl_amd/ops.py does
 * at first use, or takes them from its committed plan table). The registry is process-wide and
 * thread-safe. Workspace sizes follow the pinned choice: query mtlssl_conv2d_workspace_bytes after. */
int mtlssl_conv2d_force_config(const mtlssl_conv_desc* d, int mode, int cfg);
/* Algorithm policy for the 3x3 / stride-1 / SAME layers: 0 = always the direct implicit GEMM, 1 = by the
 * plan registry, else by the time models (default; the MTLSSL_WINOGRAD environment variable sets the
 * initial value), 2 = Winograd F(4x4,3x3) for every eligible problem. Returns the previous mode; a mode
 * outside 0..2 only queries. Process-wide. */
int mtlssl_conv2d_set_winograd(int mode);
/* Test switch (no reference counterpart). 1x1 / stride-1 layers run on the tile engine's pointwise instantiation
 * (k_conv_mfma_pw / k_conv_glds_pw: no gather arithmetic in the K loop); 0 routes them through the general gather
 * instantiation instead — same sums in the same order, bit-identical results, 12-20 % slower — so that the suite can
 * hold one against the other. Returns the previous setting; a value outside 0..1 only queries. Process-wide. */
int mtlssl_conv2d_set_pointwise(int on);
/* Row-group activity (no reference counterpart). The _xf / _ex calls with two more arguments: group_active holds one
 * byte per group of rows_per_group consecutive GEMM rows (pixels of dy; the 49 pixels of a 7x7 RoI), and a 0 is the
 * caller's PROMISE that every dy row of that group is exactly zero (an RoI whose loss scale is 0: every backward kernel
 * of a RoI tower maps a zero RoI to a zero RoI). A pointwise (1x1, stride 1) problem on the tile engine then leaves the
 * known zeros out: the filter gradient walks only the 16-row K-steps of each block's unchanged pixel range that touch an
 * active group, the input gradient runs a zero-length K loop in tiles whose rows are all inactive (the epilogue still
 * writes them). Launch grids, split boundaries and the order of every sum stay as they are and a zero product leaves an
 * fp32 accumulator unchanged, so the results are BIT-IDENTICAL to the unflagged call.
 * A 3x3 problem on a Winograd plan (F(4x4,3x3) or the whole-7-span variant) honours the flags too when one group is one
 * batch entry of the descriptor (rows_per_group == H * W; any ldy) and the launch runs on the native engine. Input
 * gradient: only the active entries' tiles are transformed, packed in ascending order into the first rows of the
 * Winograd planes; the tiles of the GEMM stack behind them leave at once, and the output transform runs on +0 for an
 * inactive entry (residual, accumulate and mask as usual). Filter gradient: the splits of the tile range stay as planned;
 * inside each split the pairs of tiles that one MFMA instruction sums are kept when either tile is active and packed to
 * the front of the split's range in ascending order — the forward's kept input transform is gathered into the workspace
 * in that layout — and each block walks the kept K-steps only. Every accumulator still sees its nonzero terms in their
 * order: bit-identical as well. One tiny index kernel per call builds the maps on the device (no host synchronisation);
 * they live at the end of the workspace (mtlssl_conv2d_workspace_bytes / _wgrad_workspace_bytes cover them).
 * Every other problem (direct 3x3, strided, the small-channel kernels, the split-bf16 engine) ignores the flags;
 * group_active = NULL is the _xf / _ex call. The pointwise filter gradient keeps its step list in the workspace
 * (mtlssl_conv2d_wgrad_workspace_bytes covers it). */
int mtlssl_conv2d_dgrad_rs(const mtlssl_conv_desc* d, const float* dy, const float* w, const float* residual,
                           const float* mask_ref, float* dx, int epilogue, void* workspace, const float* filter_xf,
                           int xf_variant, const uint8_t* group_active, int rows_per_group, mtlssl_stream_t stream);
int mtlssl_conv2d_wgrad_rs(const mtlssl_conv_desc* d, const float* x, const float* dy,
                           const float* out_scale, float* dw, float* dbias, const float* dbias_scale, float beta,
                           void* workspace, const float* input_xf, int input_variant, const uint8_t* group_active,
                           int rows_per_group, mtlssl_stream_t stream);
/* flags[i] = scale[i] != 0 for n groups: the per-RoI loss scale as the byte flags the calls above take. */
int mtlssl_row_group_flags(const float* scale, int n, uint8_t* flags, mtlssl_stream_t stream);
/* 0: the calls above ignore their flags (the A/B and test switch), 1 (default): they use them. Returns the previous
 * setting; any other value only queries. Process-wide. */
int mtlssl_conv2d_set_row_skip(int on);
/* fp32 matrix engine of the large implicit GEMMs. 0 (default; MTLSSL_FP32_ENGINE unset): v_mfma_f32_32x32x2_f32,
 * exact fp32 products with fp32 accumulation. 1 (MTLSSL_FP32_ENGINE=split): problems with at least 192 tiles of
 * 256 x 256 run on the bf16 matrix datapath with every operand split EXACTLY into three bf16 pieces (hi + mid + lo
 * = the fp32 value) and six of the nine piece products accumulated in fp32; the three dropped products are each below
 * 2^-21 |a*b| in the worst case, about 2^-24 |a*b| on average (the size of one fp32 accumulation rounding). Same error against fp64 as mode 0 (tests/test_gpu_split_engine.py), other
 * summation order (not bit-identical), +-inf operands yield NaN.
 * 2 ("high") and 3 ("medium") are REDUCED levels of the same engine, reachable through this call only (the environment
 * variable keeps its meaning: split / 1, anything else native). They trade a stated amount of accuracy for matrix rate:
 *   2: every operand truncated to 16 significant bits (bit pattern & 0xFFFFFF00) as two bf16 pieces h + m, the three
 *      products (h,h) (h,m) (m,h): |y - exact| <= (3 * 2^-14 + 2^-18) * sum|a||b| on top of mode 0's own error;
 *   3: every operand rounded to ONE bf16, round-to-nearest-even, one product: |y - exact| <= (2^-8 + 2^-18) * sum|a||b|
 *      on top of mode 0's error. +-inf operands stay inf; values within half a bf16 ulp of FLT_MAX round to inf.
 * The reduced levels apply to the DIRECT launches (forward, data gradient, direct filter gradient) of the problems
 * mode 1 takes; the Winograd-domain GEMMs run with all six products under every mode >= 1 (the Winograd transforms
 * amplify operand error about a hundredfold: no bound exists for fewer products there), and problems mode 1 leaves to
 * the native engine stay there bit for bit under every mode.
 * Returns the previous mode; -1 (and any other value outside 0..3) only queries. Process-wide. */
int mtlssl_conv2d_set_fp32_engine(int mode);
/* out[4] = tile-engine GEMM launches made with native fp32 / six / three / one product(s) since the library was loaded
 * or since the last call with reset != 0 (which returns the counts and then zeroes them). Host-side relaxed atomic
 * counters, bumped where the launch is chosen: they tell which engine ran without comparing bits. Process-wide. */
int mtlssl_conv2d_engine_launches(int64_t* out, int reset);
/* Number of launches of the implicit-GEMM kernel one call makes for this problem (2 when the planner
 * splits off a K-split tail launch) — lets a profiler relate per-call timings to
 * per-dispatch kernel traces. */
int mtlssl_conv2d_num_dispatches(const mtlssl_conv_desc* d, int mode);
/* Read-only report of what a call of (d, mode) will launch, from the same memoised planners the launch functions ask
 * (a workspace is assumed; host arithmetic only, no device is touched and no decision changes). out[MTLSSL_PLAN_INFO_LEN]:
 *   [0]  family, MTLSSL_PLAN_* below
 *   [1]  plan code, = mtlssl_conv2d_tile_config(d, mode)
 *   [2]  tile (0..7, CFG_BM x CFG_BN of [11] x [12]) of the GEMM that runs: the direct plan's, the one of the padded /
 *        space-to-depth / parity sub-problem, the Winograd GEMM stack's; -1 when no tile kernel runs
 *   [3]  nsplit: K splits of the (main) launch; wgrad: splits of the pixel range      [4] K-steps (16 deep) per split
 *   [5]  tail_rows: tile rows of the K-split tail launch (0: none)   [6] tail_nsplit   [7] K-steps per tail split
 *   [8]  K-steps of the whole reduction (a last split is ragged when [8] % [4] != 0)
 *   [9]  GEMM rows M   [10] GEMM width NG (those of the padded / sub-problem)   [11] BM   [12] BN
 *   [13] wgrad: pixels per split   [14] = mtlssl_conv2d_num_dispatches(d, mode)   [15] 0
 * The stride-2 dgrad by input parity runs four sub-problems with a plan each: parity_class 0..3 = (ih % 2) * 2 + iw % 2
 * selects one ([3] = 0 for a class without taps); the argument is ignored for every other family. */
#define MTLSSL_PLAN_INFO_LEN 16
#define MTLSSL_PLAN_DIRECT 0    /* implicit GEMM on the problem as given */
#define MTLSSL_PLAN_PADDED 1    /* pointwise problem with its reduction (wgrad: output) width zero-padded */
#define MTLSSL_PLAN_THIN 2      /* K <= 8 pointwise forward, one wavefront per pixel */
#define MTLSSL_PLAN_S2D 3       /* stride-2 stem as a stride-1 problem on the space-to-depth image */
#define MTLSSL_PLAN_PARITY 4    /* stride-2 dgrad as four stride-1 problems by input parity */
#define MTLSSL_PLAN_WINO_F43 5
#define MTLSSL_PLAN_WINO_M7 6
#define MTLSSL_PLAN_VALU 7      /* a non-MFMA fallback kernel */
int mtlssl_conv2d_plan_info(const mtlssl_conv_desc* d, int mode, int parity_class, int32_t* out);
/* Multiply-accumulates the launch plan of (d, mode) executes on the matrix cores (on_mfma = 1) or in a VALU fallback
 * kernel (on_mfma = 0): direct problems count M*N*K of the implicit GEMM, Winograd variants the transformed-domain
 * GEMM stack, padded / space-to-depth forms their zero-padded width, the input-parity stride-2 dgrad a quarter of the
 * taps. What `whole_step.executed_tflops` of bench.py is summed from (the reference has no counterpart: TensorFlow
 * 1.7 reports no FLOP counts for its cuDNN / Eigen convolutions). */
int64_t mtlssl_conv2d_executed_macs(const mtlssl_conv_desc* d, int mode, int on_mfma);
int mtlssl_conv2d_wgrad(const mtlssl_conv_desc* d, const float* x, const float* dy,
                        const float* out_scale, float* dw, float* dbias, float beta,
                        void* workspace, mtlssl_stream_t stream);

/* Grouped filter gradient: n problems of ONE descriptor in one launch — the 22 shape-identical bottleneck units of
 * ResNet-101's block3 (slim/nets/resnet_v1.py:69-130 stacked by resnet_utils.py:126-200) each give a 4 864-pixel
 * reduction at per-GPU batch 2, far too few tiles to fill 256 CUs one at a time. x_ptrs / dy_ptrs / dw_ptrs (and
 * scale_ptrs, nullable as a whole or per entry) are DEVICE arrays of n pointers; dw[g] = beta*dw[g] + scale[g][k] *
 * sum_pixels x[g]*dy[g]. MFMA-path problems only (C, K multiples of 4, >= 16); no dbias. */
int64_t mtlssl_conv2d_wgrad_grouped_workspace_bytes(const mtlssl_conv_desc* d, int n);
int mtlssl_conv2d_wgrad_grouped(const mtlssl_conv_desc* d, int n, const void* x_ptrs, const void* dy_ptrs,
                                const void* scale_ptrs, const void* dw_ptrs, float beta, void* workspace,
                                mtlssl_stream_t stream);

/* Depthwise convolution (slim.separable_conv2d with num_outputs=None, depth_multiplier 1:
 * slim/nets/mobilenet_v1.py:229-245; models/faster_rcnn_mobilenet_v1_feature_extractor.py:145-184).
 * Descriptor with C == K; filter layout [R,S,C]. Epilogue flags BIAS / RELU / RELU6 (fwd) and
 * MASK / MASK6 (dgrad). HBM-bound. */
int mtlssl_depthwise_fwd(const mtlssl_conv_desc* d, const float* x, const float* w, const float* bias,
                         float* y, int epilogue, mtlssl_stream_t stream);
int mtlssl_depthwise_dgrad(const mtlssl_conv_desc* d, const float* dy, const float* w,
                           const float* mask_ref, float* dx, int epilogue, mtlssl_stream_t stream);
int64_t mtlssl_depthwise_wgrad_workspace_bytes(const mtlssl_conv_desc* d);
int mtlssl_depthwise_wgrad(const mtlssl_conv_desc* d, const float* x, const float* dy,
                           const float* out_scale, float* dw, float beta, void* workspace,
                           mtlssl_stream_t stream);
/* Gradients of the trainable gamma/beta of an inference-mode slim.batch_norm that has been folded
 * into its producing convolution (slim/nets/mobilenet_v1.py:376-413: the MobileNet arg scope runs
 * BatchNorm with is_training=False but leaves gamma/beta trainable). y [rows,C] = the layer's
 * post-activation output, g [rows,C] = dL/d(pre-activation) (already ReLU/ReLU6-masked):
 * dbeta = colsum(g), dgamma = colsum(g*(y-beta))/gamma; `accum` != 0 adds into dgamma/dbeta. */
int64_t mtlssl_bn_param_grads_workspace_bytes(int C);
int mtlssl_bn_param_grads(const float* y, const float* g, const float* gamma, const float* beta,
                          float* dgamma, float* dbeta, int64_t rows, int C, float accum, void* workspace,
                          mtlssl_stream_t stream);

/* ------------------------------------------------------------------ batch-statistics BatchNorm
 * slim.batch_norm in TRAINING mode (fused=None, i.e. the fused kernel), the normalizer_fn that a hyperparams block with
 * `batch_norm { train: true }` installs while training (protos/hyperparams.proto:101-110,
 * builders/hyperparams_builder.py:56-76, 156-175), over x [rows, C] = the bias-free output of the layer's filter (NHWC
 * flattened: rows = all pixels, or all RoIs, of the per-GPU batch), n = rows:
 *   mean = sum(x) / n          var = sum((x - mean)^2) / n     (biased, from deviations, never E[x^2] - mean^2)
 *   inv_std = 1 / sqrt(var + eps)                               (correctly rounded fp32 sqrt and division)
 *   y = act(((x - mean) * inv_std) * gamma + beta)              gamma null: 1 (scale: false); beta null: 0 (center: false)
 * act: epilogue 0, MTLSSL_EPI_RELU or MTLSSL_EPI_RELU6. save_mean / save_inv_std [C] are what the backward reads.
 * moving_mean / moving_var [C] (both or neither) are updated in place by slim's
 * assign_moving_average(zero_debias=False), as one unfused fp32 sequence with f = float(1 - decay):
 *   moving_mean -= (moving_mean - mean) * f
 *   moving_var  -= (moving_var - (var * n) / max(n - 1, 1)) * f      (the fused kernel's Bessel-corrected output)
 * One launch, no workspace: one workgroup owns 32 channels and walks every row three times (mean, variance, normalise);
 * the per-channel partials of its 64 row lanes combine in registers and LDS in a fixed order — no atomics, two calls on
 * the same data agree bit for bit. Any rows in [1, 2^24], any C >= 1. */
int mtlssl_batch_norm_train_fwd(const float* x, const float* gamma, const float* beta, float* y, float* save_mean,
                                float* save_inv_std, float* moving_mean, float* moving_var, int64_t rows, int C,
                                float eps, float f, int epilogue, mtlssl_stream_t stream);
/* Its gradient. dy [rows, C] = dL/dy; with mask_epilogue MTLSSL_EPI_MASK (ReLU) or MTLSSL_EPI_MASK6 (ReLU6) the
 * activation's mask is taken from y (the forward's output, required then) inside: g = dy * mask(y), else g = dy.
 * With xhat = (x - save_mean) * save_inv_std:
 *   dbeta = sum(g)     dgamma = sum(g * xhat)     dx = (gamma * inv_std) * ((g - sum(g)/n) - xhat * (sum(g * xhat)/n))
 * dgamma / dbeta may be null; accum != 0: d* = accum * d* + the sum (as mtlssl_bn_param_grads). Same launch shape,
 * same determinism; dx may not alias x or dy. */
int mtlssl_batch_norm_train_bwd(const float* x, const float* dy, const float* y, const float* gamma,
                                const float* save_mean, const float* save_inv_std, float* dx, float* dgamma,
                                float* dbeta, int64_t rows, int C, float accum, int mask_epilogue,
                                mtlssl_stream_t stream);

/* slim.avg_pool2d with TF 'SAME'/'VALID' semantics — the divisor is the number of in-bounds
 * cells of each window (slim/nets/inception_resnet_v2.py:181-184, Mixed_5b Branch_3). */
int mtlssl_avgpool_fwd(const float* x, float* y, int N, int H, int W, int C, int k, int stride, int pad_t,
                       int pad_l, int OH, int OW, mtlssl_stream_t stream);
int mtlssl_avgpool_bwd(const float* dy, float* dx, int N, int H, int W, int C, int k, int stride, int pad_t,
                       int pad_l, int OH, int OW, mtlssl_stream_t stream);
/* tf.concat(axis=3) and its gradient as channel-slice copies (slim/nets/inception_resnet_v2.py:46,
 * 67,88,185-186,213,253): dst[row, dst_c0 + j] (=|+=) src[row, src_c0 + j] for j < nc. */
int mtlssl_copy_channels(const float* src, int src_ld, int src_c0, float* dst, int dst_ld, int dst_c0,
                         int64_t rows, int nc, int accumulate, mtlssl_stream_t stream);

/* slim.max_pool2d (slim/nets/resnet_v1.py:222; resnet_utils.subsample :59-74). */
int mtlssl_maxpool_fwd(const float* x, float* y, int N, int H, int W, int C, int k, int stride,
                       int pad_t, int pad_l, int OH, int OW, mtlssl_stream_t stream);
int mtlssl_maxpool_bwd(const float* x, const float* y, const float* dy, float* dx, int N, int H,
                       int W, int C, int k, int stride, int pad_t, int pad_l, int OH, int OW,
                       mtlssl_stream_t stream);
/* The pooling branch of a tf.concat(axis=3) (Mixed_6a / Mixed_7a Branch_2 / Branch_3, slim/nets/inception_resnet_v2.py:
 * 200-213, 240-253): y (forward) and y / dy (backward) are the channel slice [c0, c0+C) of a wider NHWC map with `ldy`
 * channels per pixel, the pointers already at channel c0; x / dx are dense. C % 4 == 0, ldy % 4 == 0, 16-byte aligned
 * pointers, k in {2, 3}; the backward is the overlapping-window gather (k > stride). */
int mtlssl_maxpool_fwd_strided(const float* x, float* y, int N, int H, int W, int C, int k, int stride,
                               int pad_t, int pad_l, int OH, int OW, int ldy, mtlssl_stream_t stream);
int mtlssl_maxpool_bwd_strided(const float* x, const float* y, const float* dy, float* dx, int N, int H,
                               int W, int C, int k, int stride, int pad_t, int pad_l, int OH, int OW, int ldy,
                               mtlssl_stream_t stream);
/* tf.reduce_mean over H,W (core/box_predictor.py:469-471) and its gradient. */
int mtlssl_spatial_mean_fwd(const float* x, float* y, int N, int HW, int C, mtlssl_stream_t s);
int mtlssl_spatial_mean_bwd(const float* dy, float* dx, int N, int HW, int C, mtlssl_stream_t s);
/* The same fused with the activation gradient of the averaged tensor `act` [N,HW,C] (the tower output
 * is a ReLU / ReLU6 output): dx = (0 < act (< 6)) ? dy/HW : 0. */
int mtlssl_spatial_mean_bwd_masked(const float* dy, const float* act, float* dx, int N, int HW, int C,
                                   int relu6, mtlssl_stream_t stream);

/* ------------------------------------------------------------------ detection family */

/* GridAnchorGenerator._generate / tile_anchors
 * (anchor_generators/grid_anchor_generator.py:96-214). scales/aspect_ratios are HOST arrays. */
int mtlssl_anchors_generate(float* anchors_out, int grid_h, int grid_w, const float* scales,
                            int n_scales, const float* aspect_ratios, int n_ratios, float base_h,
                            float base_w, float stride_y, float stride_x, float offset_y,
                            float offset_x, mtlssl_stream_t stream);

/* box_list_ops.prune_outside_window (core/box_list_ops.py:140-169): order-preserving
 * compaction. keep_idx_out[n] int32, count_out[1] int32 (device). */
int mtlssl_boxes_prune_outside_window(const float* boxes, int n, float win_ymin, float win_xmin,
                                      float win_ymax, float win_xmax, int32_t* keep_idx_out,
                                      int32_t* count_out, mtlssl_stream_t stream);

/* box_list_ops.clip_to_window(filter_nonoverlapping=False) (core/box_list_ops.py:102-137): the
 * inference-time anchor clipping of faster_rcnn_meta_arch.py:583-585 (grid anchors always overlap
 * the image, so the reference's empty-box filter never removes one). */
int mtlssl_boxes_clip_to_window(const float* boxes, int n, float win_ymin, float win_xmin, float win_ymax,
                                float win_xmax, float* out, mtlssl_stream_t stream);
/* tf.gather over rows per batch item (faster_rcnn_meta_arch.py:965-976) and its gradient
 * (scatter into a zeroed buffer; indices are unique). */
int mtlssl_gather_rows(const float* src, const int32_t* idx, float* dst, int batch, int n_src,
                       int n_idx, int row_len, mtlssl_stream_t stream);
int mtlssl_scatter_rows(const float* src, const int32_t* idx, float* dst, int batch, int n_dst,
                        int n_idx, int row_len, mtlssl_stream_t stream);

/* FasterRcnnBoxCoder._decode/_encode (box_coders/faster_rcnn_box_coder.py:60-118);
 * anchors are broadcast over `batch` when anchors_batched == 0. */
int mtlssl_boxes_decode(const float* rel_codes, const float* anchors, float* boxes_out, int batch,
                        int n, int anchors_batched, float sy, float sx, float sh, float sw,
                        mtlssl_stream_t stream);
int mtlssl_boxes_encode(const float* boxes, const float* anchors, float* codes_out, int n, float sy,
                        float sx, float sh, float sw, mtlssl_stream_t stream);

/* _postprocess_rpn (faster_rcnn_meta_arch.py:1055-1115) =
 * decode + softmax fg score + score filter + clip_to_window + greedy NMS + sort + pad.
 * Outputs: proposals_out [B,max_proposals,4] ABSOLUTE coords zero padded,
 * scores_out [B,max_proposals], num_out int32[B].
 * workspace: mtlssl_rpn_proposals_workspace_bytes(B, n). */
int64_t mtlssl_rpn_proposals_workspace_bytes(int batch, int n);
int mtlssl_rpn_proposals(const float* rpn_box_encodings, const float* rpn_objectness,
                         const float* anchors, int batch, int n, float img_h, float img_w,
                         float score_thresh, float iou_thresh, int max_proposals,
                         float* proposals_out, float* scores_out, int32_t* num_out,
                         void* workspace, mtlssl_stream_t stream);
/* Inference post-processing: batch_multiclass_non_max_suppression (core/post_processing.py:167-312 over
 * multiclass_non_max_suppression :25-164) as called by FasterRCNNMetaArch._postprocess_box_classifier
 * (meta_architectures/faster_rcnn_meta_arch.py:1387-1469). boxes [B,n,q,4] (q == 1 or num_classes),
 * scores [B,n,num_classes] with row stride scores_ld >= num_classes (already score-converted; pass
 * the pointer to column 1 of a [B,n,num_classes+1] tensor to drop the background slot like
 * tf.slice does at :1441-1444), num_valid int32[B] or NULL. Per class: score
 * filter (strict >), clip to clip_window (4 floats in HOST memory; NULL = no clipping) dropping empty boxes, optional
 * change_coordinate_frame, greedy NMS capped at max_per_class; then all classes merged, sorted by
 * score (stable), capped at max_total and zero padded. classes_out holds 0-based class ids as floats
 * like the reference; num_out int32[B]. The host-side check text of the reference's ValueErrors is
 * kept in the error messages. */
int64_t mtlssl_batch_multiclass_nms_workspace_bytes(int batch, int n, int num_classes, int max_per_class);
int mtlssl_batch_multiclass_nms(const float* boxes, const float* scores, int scores_ld,
                                const int32_t* num_valid, int batch, int n, int q, int num_classes,
                                float score_thresh,
                                float iou_thresh, int max_per_class, int max_total,
                                const float* clip_window, int change_coordinate_frame, float* boxes_out,
                                float* scores_out, float* classes_out, int32_t* num_out, void* workspace,
                                mtlssl_stream_t stream);
/* Score converters of builders/post_processing_builder.py:80-108: mode 1 = tf.nn.softmax over the last
 * axis, mode 2 = tf.sigmoid. logits/out [rows, C]. */
int mtlssl_score_convert(const float* logits, float* out, int64_t rows, int C, int mode,
                         mtlssl_stream_t stream);
/* Stand-alone pieces of the above, exposed for parity tests:
 * greedy NMS of tf.image.non_max_suppression (call site core/post_processing.py:146) on
 * boxes that are already filtered (finite scores); selected_out[max_out] int32 indices in selection order. */
int64_t mtlssl_nms_workspace_bytes(int n);
int mtlssl_nms(const float* boxes, const float* scores, int n, float iou_thresh, int max_out,
               int32_t* selected_out, int32_t* num_out, void* workspace,
               mtlssl_stream_t stream);

/* Evaluation (mtl_ssl_amd/eval.py), no training counterpart.
 * Per-class re-suppression of postprocessed detections inside the evaluator: eval_config.nms_type / nms_threshold /
 * soft_nms_sigma (utils/per_image_evaluation.py:35-68, 258; utils/object_detection_evaluation.py:45-59, 294-357) with
 * the semantics of utils/np_box_list_ops.py: nms_type 1 = non_max_suppression (:185-258), 2 / 3 =
 * soft_non_max_suppression linear / Gaussian (:259-366), score filter > -10, iou_threshold == 1.0 = sort and cap only.
 * One workgroup per segment: segment s is rows [segment_offsets[s], segment_offsets[s+1]) of boxes [N,4] (fp32, times
 * scale_y / scale_x in double like the host evaluator) and scores [N] (fp32); segment_offsets int32[num_segments+1]
 * in device memory; max_segment = the largest segment length (host int), at most MTLSSL_EVAL_NMS_MAX_SEGMENT (the
 * segment is held in LDS). IoU, weights and the Gaussian exp (csrc/portable_math.h) are evaluated in double;
 * every rescale rounds once to fp32. Outputs per segment, in its own rows: index_out = segment-local input indices in
 * output order, scores_out = their (rescored) scores, count_out[s] = how many; rows past the count hold -1 / 0.
 * Thresholds and scales are doubles (the evaluator's numpy arithmetic). */
#define MTLSSL_EVAL_NMS_MAX_SEGMENT 1024
#define MTLSSL_EVAL_NMS_STANDARD 1
#define MTLSSL_EVAL_NMS_SOFT_LINEAR 2
#define MTLSSL_EVAL_NMS_SOFT_GAUSSIAN 3
int mtlssl_eval_nms(const float* boxes, const float* scores, const int32_t* segment_offsets, int num_segments,
                    int max_segment, int nms_type, double iou_threshold, double sigma, double scale_y, double scale_x,
                    int max_output, int32_t* index_out, float* scores_out, int32_t* count_out,
                    mtlssl_stream_t stream);
/* The edge-mask metric's per-pixel work for one image (utils/mtl_util.py:91-101): logits [Hf,Wf,2] resized to
 * [h,w] as skimage.transform.resize(x, (h, w, 2)) does at order 1 in scikit-image 0.13 / 0.14 (pixel (r, c) samples
 * ((r+0.5)*Hf/h - 0.5, (c+0.5)*Wf/w - 0.5), bilinear, outside the map reads 0, no anti-aliasing), each channel rounded
 * to fp32, label = ch0 < ch1; count_out (one int32, device) = pixels whose label equals gt_mask [h,w]. */
int mtlssl_edgemask_agreement(const float* logits, int Hf, int Wf, const float* gt_mask, int h, int w,
                              int32_t* count_out, mtlssl_stream_t stream);
/* The MS-COCO evaluator's greedy match (pycocotools COCOeval.evaluateImg as restated by CocoDetectionEvaluator._iou /
 * _evaluate_image in mtl_ssl_amd/evaluation.py, which define the semantics; the reference reaches it through
 * utils/object_detection_evaluation.py:294-425). A segment is one (image, category) pair with at least one detection
 * or groundtruth box: detections [dt_off[s], dt_off[s+1]) of dt_boxes [ND,4] and groundtruth [gt_off[s], gt_off[s+1])
 * of gt_boxes [NG,4] / gt_area [NG] / gt_crowd [NG] (offsets int32[num_segments+1]; boxes ymin,xmin,ymax,xmax in
 * pixels, double; everything in device memory). The caller has sorted each segment's detections by descending score,
 * stably, and cut them to the image's best max_detections_per_image. iou_thrs [T] and area_rng [A,2] are the
 * evaluator's own doubles; T*A <= 64. One wavefront per segment, lane t*A + a walks the detections in order for
 * threshold t in area range a: the unclaimed box of highest IoU >= min(thr, 1 - 1e-10) (an equal IoU replaces),
 * regular boxes before ignored ones (crowd, or area outside [lo, hi]), crowd boxes claimable again with IoU =
 * intersection / detection area, union floored at 1e-300. Outputs: bit t*A + a of dt_match[i] / dt_ignore[i] =
 * detection i matched / is ignored (matched to an ignored box, or unmatched with its own area outside the range);
 * npig[s*A + a] = the segment's groundtruth boxes not ignored in range a. The first m detections of a segment are the
 * result for maxDets = m. max_gt = the largest groundtruth count of a segment (host int), at most
 * MTLSSL_COCO_MATCH_MAX_GT; beyond it MTLSSL_EINVAL (the evaluator keeps such a segment on the host). All arithmetic
 * in double, plain stores, no atomics: the same bits run to run. */
#define MTLSSL_COCO_MATCH_MAX_GT 256
int mtlssl_coco_match(const int32_t* dt_off, const int32_t* gt_off, int num_segments, int max_gt,
                      const double* dt_boxes, const double* gt_boxes, const double* gt_area, const uint8_t* gt_crowd,
                      const double* iou_thrs, int num_iou_thrs, const double* area_rng, int num_area_rng,
                      uint64_t* dt_match, uint64_t* dt_ignore, int32_t* npig, mtlssl_stream_t stream);
/* The PASCAL evaluator's tp/fp labelling for every groundtruth subset at once (utils/per_image_evaluation.py:233-281,
 * which utils/object_detection_evaluation.py:199-211 runs once per subset with groundtruth_is_difficult = ~member;
 * restated by PascalDetectionEvaluator._tp_fp in mtl_ssl_amd/evaluation.py, which defines the semantics). A segment is
 * one (image, class) pair that holds a detection: detections [dt_off[s], dt_off[s+1]) of dt_boxes [ND,4] and
 * groundtruth [gt_off[s], gt_off[s+1]) of gt_boxes [NG,4] / gt_member [NG] (offsets int32[num_segments+1]; boxes
 * ymin,xmin,ymax,xmax, double; bit j of gt_member = the box belongs to subset j; everything in device memory). The
 * caller has filtered, sorted and capped each segment's detections exactly as _tp_fp does. One wavefront per segment:
 * per detection the IoUs against every groundtruth box in utils/np_box_ops.py's double arithmetic (np.maximum /
 * np.minimum with NaN propagation, inter / ((area_a + area_b) - inter), no floor: 0/0 is NaN), np.argmax's box g (the
 * first NaN if there is one, otherwise the first maximum), then lane j < num_subsets with its own claimed set: IoU >=
 * iou_threshold and g outside subset j -> bit j of drop[i] (the detection is removed from subset j); IoU >= threshold,
 * g a member and unclaimed -> bit j of tp[i], g claimed; otherwise a false positive (no bit). hit[i] = 1 when the best
 * IoU >= threshold whatever the membership (CorLoc reads it), else 0. Every element of tp / drop / hit [ND] is written.
 * max_gt = the largest groundtruth count of a segment (host int), at most MTLSSL_PASCAL_MATCH_MAX_GT, and num_subsets at
 * most 64; beyond either MTLSSL_EINVAL (the evaluator keeps such work on the host). A segment that breaks the bound
 * all the same gets hit = MTLSSL_PASCAL_MATCH_LEFT_OUT. Plain stores, no atomics: the same bits run to run. */
#define MTLSSL_PASCAL_MATCH_MAX_GT 256
#define MTLSSL_PASCAL_MATCH_LEFT_OUT 2
int mtlssl_pascal_match(const int32_t* dt_off, const int32_t* gt_off, int num_segments, int max_gt,
                        const double* dt_boxes, const double* gt_boxes, const uint64_t* gt_member,
                        double iou_threshold, int num_subsets, uint64_t* tp, uint64_t* drop, uint8_t* hit,
                        mtlssl_stream_t stream);

/* Auxiliary-task labels from the groundtruth alone (Trainer(aux_labels="generate")): what the reference computes once,
 * offline, when it writes a record (create_records/create_pascal_tf_record.py:120-421), made per step on the device
 * from the padded tensors the model holds after provide_groundtruth: boxes_norm [B,max_gt,4] (normalised), classes_bg
 * [B,max_gt,K+1] (one-hot, column 0 = background and zero), num int32[B] (rows >= num[b] are never read). height /
 * width: the size in pixels of the (resized) image the boxes are relative to; absolute box = (double)normalised * size.
 * All arithmetic in double, each output rounded once to fp32, every reduction in a fixed order (no atomics): the same
 * bits run to run. Host definitions: mtl_ssl_amd/labels.py draw_windows / window_labels_exact /
 * closeness_labels_exact / edgemask_exact. The label kernels keep an image's boxes in LDS: max_gt is at most
 * MTLSSL_AUX_MAX_GT, beyond it they return MTLSSL_EINVAL. */
#define MTLSSL_AUX_MAX_GT 256
#define MTLSSL_AUX_WINDOW_ATTEMPTS 100
/* create_multi_object, random_multi_object branch (create_pascal_tf_record.py:225-261), with Python's sequential
 * random.random() replaced by the counter hash: uniform j of window slot w, attempt a of image b is
 * (mix32(seed', 0x57494E44, (w * 100 + a) * 4 + j) >> 8) * 2^-24, seed' = mix32(mix32(seed, 0x57494E44, step),
 * 0x57494E44, image0 + b). A window that has no intersection of positive area with any box is redrawn, at most
 * MTLSSL_AUX_WINDOW_ATTEMPTS times per slot (the last draw is kept); an image without boxes repeats its first window.
 * window_boxes [B,num_windows,4] normalised; bit-exact against labels.draw_windows. */
int mtlssl_aux_draw_windows(const float* boxes_norm, const int32_t* num, int batch, int max_gt, int num_windows,
                            double height, double width, double min_obj_size, uint32_t seed, uint32_t step,
                            uint32_t image0, float* window_boxes, mtlssl_stream_t stream);
/* get_multi_label with label_option 1 / normalize_option 1 (create_pascal_tf_record.py:199-226) over
 * get_rect_area_total (:140-162): per (image, window) the exact area of the union of each present class's boxes
 * clipped to the window (slab sweep over the sorted x edges, intervals merged in y), of all boxes for the background
 * slot, then sqrt and division by the sum. window_boxes [B,num_windows,4] normalised (an input, so that recorded
 * windows can be labelled too); labels_out [B,num_windows,K+1]. One workgroup per (image, window). */
int mtlssl_aux_window_labels(const float* boxes_norm, const float* classes_bg, const int32_t* num,
                             const float* window_boxes, int batch, int max_gt, int num_classes, int num_windows,
                             double height, double width, float* labels_out, mtlssl_stream_t stream);
/* get_closeness (create_pascal_tf_record.py:325-358): per object and OTHER class 1 - centre distance / image diagonal
 * of the nearest instance, background slot 1 when nothing of another class is around (a single object included),
 * normalised to sum 1. closeness_out [B,max_gt,K+1], rows >= num[b] zero. */
int mtlssl_aux_closeness(const float* boxes_norm, const float* classes_bg, const int32_t* num, int batch, int max_gt,
                         int num_classes, double height, double width, float* closeness_out, mtlssl_stream_t stream);
/* create_edgemask (create_pascal_tf_record.py:375-421): cell ranges with its int() truncations, the +0.99 and the
 * zero-width fix-ups; plane 0 = covered by a box, plane 1 = max(1/mask^2, max over covering boxes of 1/bw/bh) divided
 * by its mean (accumulated in double). edgemask_out [B,2,mask_size,mask_size]; the reference's mask_size is 64. */
int mtlssl_aux_edgemask(const float* boxes_norm, const int32_t* num, int batch, int max_gt, double height, double width,
                        int mask_size, float* edgemask_out, mtlssl_stream_t stream);

/* TargetAssigner.assign with IouSimilarity + ArgMaxMatcher
 * (core/target_assigner.py:99-213, matchers/argmax_matcher.py:102-189,
 * core/region_similarity_calculator.py:57-74). One call handles a batch:
 *   anchors [n,4] shared (anchors_batched=0) or [B,n,4];
 *   gt_boxes [B,max_gt,4] absolute, num_gt int32[B];
 *   gt_labels [B,max_gt,label_dim] (nullable -> label 1, label_dim must be 1);
 *   gt_extra  [B,max_gt,extra_dim] (closeness, nullable);
 *   unmatched_cls_target [label_dim] (device).
 * Outputs (any nullable): match int32[B,n] in {-2,-1,0..G-1}; cls_targets [B,n,label_dim];
 * cls_weights [B,n]; reg_targets [B,n,4]; reg_weights [B,n]; extra_targets [B,n,extra_dim].
 * workspace: mtlssl_assign_targets_workspace_bytes(B, n, max_gt). */
int64_t mtlssl_assign_targets_workspace_bytes(int batch, int n, int max_gt);
int mtlssl_assign_targets(const float* anchors, int anchors_batched, int batch, int n,
                          const float* gt_boxes, const int32_t* num_gt, int max_gt,
                          const float* gt_labels, int label_dim, const float* gt_extra,
                          int extra_dim, const float* unmatched_cls_target, float matched_thresh,
                          float unmatched_thresh, int force_match, int32_t* match_out,
                          float* cls_targets_out, float* cls_weights_out, float* reg_targets_out,
                          float* reg_weights_out, float* extra_targets_out, void* workspace,
                          mtlssl_stream_t stream);

/* BalancedPositiveNegativeSampler.subsample (core/balanced_positive_negative_sampler.py:51-92)
 * with tf.random_shuffle replaced by counter-hash priorities (seed, stream_id0 + batch index
 * * stream_stride). indicator/labels/sampled_out are float 0/1 arrays [B,n]. */
int mtlssl_balanced_sample(const float* indicator, const float* labels, int batch, int n,
                           int batch_size, float positive_fraction, uint32_t seed,
                           uint32_t stream_id0, uint32_t stream_stride, float* sampled_out,
                           mtlssl_stream_t stream);

/* _unpad_proposals_and_sample_box_classifier_batch + _sample_box_classifier_minibatch
 * (faster_rcnn_meta_arch.py:1134-1216,1268-1302): detector-assign the valid proposals,
 * balanced-sample, keep order, zero pad to n2. proposals [B,max_p,4] absolute.
 * Outputs: boxes_abs_out [B,n2,4], boxes_norm_out [B,n2,4], num_out int32[B]. */
int mtlssl_sample_proposals(const float* proposals, const int32_t* num_proposals, int batch,
                            int max_p, const float* gt_boxes, const int32_t* num_gt, int max_gt,
                            const float* gt_labels_bg, int label_dim, int n2,
                            float balance_fraction, uint32_t seed, uint32_t stream_id0,
                            uint32_t stream_stride, float img_h, float img_w,
                            float* boxes_abs_out, float* boxes_norm_out, int32_t* num_out,
                            mtlssl_stream_t stream);

/* tf.image.crop_and_resize (bilinear, extrapolation 0) fused with the VALID k x k / stride
 * max-pool that follows it (faster_rcnn_meta_arch.py:1304-1348).
 * feat [B,H,W,C]; boxes [R,4] normalised; box_ind int32[R];
 * out [R,PH,PW,C] with PH = (crop-k)/stride+1; argmax_out uint8 [R,PH,PW,C] (nullable; index
 * of the winning crop sample inside its pool window, needed by the backward). */
int mtlssl_roi_crop_pool_fwd(const float* feat, int B, int H, int W, int C, const float* boxes,
                             const int32_t* box_ind, int R, int crop, int pool_k, int pool_stride,
                             float* out, uint8_t* argmax_out, mtlssl_stream_t stream);
/* dfeat += scatter(dout) (dfeat must be zeroed or hold an accumulated gradient). */
int mtlssl_roi_crop_pool_bwd(const float* dout, const uint8_t* argmax, int B, int H, int W, int C,
                             const float* boxes, const int32_t* box_ind, int R, int crop,
                             int pool_k, int pool_stride, float* dfeat, mtlssl_stream_t stream);
/* The same gradient (tf.image.crop_and_resize + max_pool2d backward, faster_rcnn_meta_arch.py:1340-1348) with the
 * accumulation behaviour and the algorithm selectable:
 *   accumulate  1: dfeat += scatter(dout) (the entry point above); 0: dfeat = scatter(dout), every element of
 *               dfeat [B,H,W,C] is written, so the caller needs no memset;
 *   algo        0: auto — the LDS-resident kernel whenever C % 16 == 0 and a workspace is given: one block per
 *               (image, 16-channel slice, band of rows) keeps its piece of the map in LDS as 64-bit fixed-point
 *               sums (step = max|dout| * 2^-30, integer adds commute), walks the image's RoIs and writes the piece
 *               once — no HBM atomics, run-to-run bit-identical; else HBM fp32 atomics;
 *               1: require the LDS-resident kernel (MTLSSL_EINVAL if the shape does not fit it);
 *               2: force the HBM-atomics kernel (order of additions, hence the last bits, varies between runs;
 *               this is what mtlssl_roi_crop_pool_bwd runs).
 *   workspace   mtlssl_roi_crop_pool_bwd_workspace_bytes() bytes of device memory (may be NULL for algo 2).
 * box_ind may be in any order. A non-finite value in dout turns the whole map into NaN (LDS kernel). */
int64_t mtlssl_roi_crop_pool_bwd_workspace_bytes(void);
int mtlssl_roi_crop_pool_bwd_ex(const float* dout, const uint8_t* argmax, int B, int H, int W, int C,
                                const float* boxes, const int32_t* box_ind, int R, int crop, int pool_k,
                                int pool_stride, float* dfeat, int accumulate, int algo, void* workspace,
                                mtlssl_stream_t stream);

/* ops.position_sensitive_crop_regions(global_pool=True) (utils/ops.py:462-609; call sites
 * core/box_predictor.py:228-264,312-330): fmap [B,H,W,C] with C = bins_y*bins_x*Cc; out [R,Cc].
 * The backward accumulates into dfmap (caller zeroes it or passes an accumulated gradient). */
int mtlssl_psroi_fwd(const float* fmap, int B, int H, int W, int C, const float* boxes,
                     const int32_t* box_ind, int R, int crop_h, int crop_w, int bins_y, int bins_x,
                     float* out, mtlssl_stream_t stream);
int mtlssl_psroi_bwd(const float* dout, int B, int H, int W, int C, const float* boxes,
                     const int32_t* box_ind, int R, int crop_h, int crop_w, int bins_y, int bins_x,
                     float* dfmap, mtlssl_stream_t stream);

/* tf.image.resize_images bilinear, align_corners=False (faster_rcnn_meta_arch.py:1870). */
int mtlssl_resize_bilinear_fwd(const float* x, float* y, int N, int H, int W, int C, int OH,
                               int OW, mtlssl_stream_t stream);
int mtlssl_resize_bilinear_bwd(const float* dy, float* dx, int N, int H, int W, int C, int OH,
                               int OW, mtlssl_stream_t stream);

/* Input-pipeline image preparation (the reference's queue runners: decode -> core/preprocessor.py:239-345
 * random_horizontal_flip -> core/preprocessor.py:1408-1411 tf.image.resize_images), after the host has decoded B
 * uint8 HWC RGB images into one buffer: out [B,OH,OW,3] float32 (0..255) = bilinear legacy resize of the image,
 * mirrored left-right first when `flip` is set; the plain cast (+ flip) when H == OH and W == OW. sy / sx are the
 * scales float32(H / OH) and float32(W / OW) computed by the caller (mtl_ssl_amd.preprocessor.resize_bilinear_legacy
 * rounds the double quotient once), so host and device agree to the bit. `desc` (device memory) holds B entries;
 * image n's pixels are pixels[desc[n].offset, + H*W*3). B <= 65535. */
typedef struct {
  int64_t offset;            /* byte offset of the image in `pixels` */
  int32_t H, W;              /* source size, >= 1 */
  int32_t flip;              /* nonzero: mirror left-right before the resize */
  float sy, sx;              /* float32(H / OH), float32(W / OW) */
  int32_t pad;
} mtlssl_image_desc;         /* 32 bytes */
int mtlssl_prepare_images(const uint8_t* pixels, const mtlssl_image_desc* desc, int B, int OH, int OW, float* out,
                          mtlssl_stream_t stream);
/* mtlssl_prepare_images with the augmentations of core/preprocessor.py (normalize_image :120, subtract_channel_mean
 * :1490, random_adjust_brightness / contrast / hue / saturation :459-540, random_distort_color :542, random_rgb_to_gray
 * :430, random_pixel_value_scale :347, random_black_patches :1189, random_crop_image :757, random_pad_image :856,
 * random_crop_pad_image :959, ssd_random_crop :1548) and random_horizontal_flip applied at the source resolution before
 * the resize, in config order. `prog` (HOST memory) holds n_ops <= 128 op codes, the same for every image; `params`
 * (device) holds B x P float32 parameters, P the sum of the ops' parameter counts (mtl_ssl_amd.preprocessor: OP_*
 * codes, OP_PARAMS counts, plan() fills them, apply_program restates every op on the host). Two ops move the frame:
 * OP_CROP (y0, x0, h, w: integers held exactly in float32; the identity crop is 0, 0, H, W) and OP_PAD (offset y,
 * offset x, target h, target w, colour mode, r, g, b; mode 0: the given colour, otherwise the mean of the frame the pad
 * receives). desc[n].flip mirrors the source before the program; desc[n].H / W stay the SOURCE size; desc[n].sy / sx
 * are float32(final H / OH), float32(final W / OW) of the frame after the whole program (the source size when no op
 * moves it). Each output tap is walked back through the program to a source pixel or a pad colour and takes the ops of
 * the stages it passes, each with the coordinate and frame width of its own stage, so the result equals
 * resize_bilinear_legacy(apply_program(image)) to the bit and no read leaves the H x W source. Every contrast op and
 * every pad op is a mean slot: two small launches compute the per-channel means of the frame of its stage in float64
 * (row sums, then rows ascending; a pad with a given colour returns at once) into `workspace`, which must hold
 * mtlssl_prepare_images_aug_workspace(B, contrast ops + pad ops, max_H) bytes, max_H >= the tallest frame of any stage
 * of any image. An empty program gives mtlssl_prepare_images's output. */
int64_t mtlssl_prepare_images_aug_workspace(int B, int n_slots, int max_H);
int mtlssl_prepare_images_aug(const uint8_t* pixels, const mtlssl_image_desc* desc, int B, int OH, int OW,
                              const int32_t* prog, int n_ops, const float* params, int P, int max_H, void* workspace,
                              int64_t workspace_bytes, float* out, mtlssl_stream_t stream);

/* ------------------------------------------------------------------ loss family
 * Fused loss + gradient. Every loss is a weighted sum of per-row terms; `row_loss_out[rows]`
 * receives the per-row contribution (already multiplied by row_scale) and
 * mtlssl_reduce_sum folds it deterministically. d* outputs are d(loss)/d(input). */

/* WeightedSmoothL1LocalizationLoss (core/losses.py:169-196):
 * row term = row_scale[r] * sum_j smoothl1(pred[r,j]-target[r,j]; sigma). */
int mtlssl_smooth_l1_fwd_bwd(const float* pred, const float* target, const float* row_scale,
                             int rows, int code_size, float sigma, float* row_loss_out,
                             float* dpred_out, mtlssl_stream_t stream);
/* WeightedSoftmaxClassificationLoss(_v2) (core/losses.py:285-352):
 * row term = row_scale[r] * -(sum_c t[r,c] * log_softmax(x[r,:])[c]) over the class columns
 * [col0, col0+C) of rows with leading dimension ld_logits / ld_targets.
 * dlogits (same ld as logits) gets row_scale*(softmax*sum(t) - t) in those columns. */
int mtlssl_softmax_ce_fwd_bwd(const float* logits, int ld_logits, const float* targets,
                              int ld_targets, int col0, int C, const float* row_scale, int rows,
                              float* row_loss_out, float* dlogits_out, mtlssl_stream_t stream);
/* out[0] = scale * sum(x[0..n)) with a fixed reduction order. */
int mtlssl_reduce_sum(const float* x, int n, float scale, float* out, mtlssl_stream_t stream);

/* ------------------------------------------------------------------ optimizer family
 * slim.learning.clip_gradient_norms (per-variable tf.clip_by_norm, slim/learning.py:282-301)
 * + tf.train.MomentumOptimizer (builders/optimizer_builder.py:48-52):
 *   g <- grad_scale*grad + var_weight_decay[v]*w  (L2 regulariser gradient, nullable table);
 *   g <- var_grad_mult[v]*g  (nullable table: trainer.py:389-405 grad_multiplier / divide_grad_by_batch /
 *        bias_grad_multiplier; a NEGATIVE entry freezes the variable — it is left out of the update like
 *        utils/variables_helper.py:100-118 leaves it out of apply_gradients, trainer.py:408-410);
 *   g <- g * min(1, clip/||g||_2) per variable; acc <- momentum*acc + g; w <- w - lr*acc.
 * The parameters live in one flat buffer; var_offsets int32[num_vars+1] (device) delimits the
 * variables (offsets in floats, multiples of 4); max_var_size = largest variable (floats).
 * norms_ws: workspace of mtlssl_sgd_workspace_bytes(num_vars, max_var_size) bytes (per-variable
 * norms + per-chunk partial sums: the norm is reduced in a fixed order, so replicas that apply the
 * same reduced gradient stay bit-identical). */
int64_t mtlssl_sgd_workspace_bytes(int num_vars, int64_t max_var_size);
int mtlssl_sgd_momentum_clip(float* weights, const float* grads, float* accum,
                             const int32_t* var_offsets, int num_vars, int64_t total,
                             int64_t max_var_size, float lr, float momentum, float clip_norm,
                             float grad_scale, const float* var_weight_decay, const float* var_grad_mult,
                             float* norms_ws, mtlssl_stream_t stream);
/* The same update that also refreshes the shadow weights of mtlssl_fold_scales (eff = w * scale[channel] for the
 * variables with a registered scale vector; same tables) on the values it already holds. Only valid when no scale
 * vector depends on a variable of this update — every BatchNorm frozen, the reference's configs for ResNet and
 * Inception-ResNet-v2 (faster_rcnn.proto batch_norm_trainable default false). eff == NULL: plain update.
 * zero_grads != 0: the launch leaves zeros in `grads` (every element, frozen variables included) — the update is the
 * gradient buffer's last reader of a step, so the next step's accumulation needs no separate memset. */
int mtlssl_sgd_momentum_clip_fold(float* weights, float* grads, float* accum,
                                  const int32_t* var_offsets, int num_vars, int64_t total,
                                  int64_t max_var_size, float lr, float momentum, float clip_norm,
                                  float grad_scale, const float* var_weight_decay, const float* var_grad_mult,
                                  float* norms_ws, float* eff, const void* scale_ptrs, const int32_t* scale_len,
                                  int zero_grads, mtlssl_stream_t stream);
/* The other two optimizers of builders/optimizer_builder.py:40-62 behind the same gradient pipeline (L2 term,
 * multipliers / frozen variables, per-variable clip; same tables and workspace as above). kind 1 =
 * tf.train.RMSPropOptimizer: slot0 = mean square (TensorFlow initialises it to ONE), slot1 = momentum;
 * p0 = decay, p1 = momentum, p2 = epsilon: ms <- p0*ms + (1-p0)*g^2; mom <- p1*mom + lr*g/sqrt(ms+p2); w <- w - mom.
 * kind 2 = tf.train.AdamOptimizer: slot0 = m, slot1 = v; p0 = beta1, p1 = beta2, p2 = epsilon; `lr` is the
 * bias-corrected rate lr*sqrt(1-beta2^t)/(1-beta1^t) of step t: w <- w - lr*m/(sqrt(v)+p2). */
int mtlssl_adaptive_update_clip(int kind, float* weights, const float* grads, float* slot0, float* slot1,
                                const int32_t* var_offsets, int num_vars, int64_t total, int64_t max_var_size,
                                float lr, float p0, float p1, float p2, float clip_norm, float grad_scale,
                                const float* var_weight_decay, const float* var_grad_mult, float* norms_ws,
                                mtlssl_stream_t stream);

/* Batched fold of per-output-channel scales into a shadow copy of the flat parameter buffer, one
 * launch for every convolution of the model: eff[i] = weights[i] * scale_v[(i - var_offsets[v]) %
 * scale_len[v]] for each variable v whose entry of `scale_ptrs` (device array of num_vars device
 * pointers) is non-null; other variables are left untouched. Replaces the per-layer
 * slim.batch_norm(is_training=False) multiply of slim/nets/resnet_v1.py:102-119 (and the residual
 * scale of slim/nets/inception_resnet_v2.py:47-52) after each optimizer step. */
int mtlssl_fold_scales(const float* weights, float* eff, const int32_t* var_offsets, int num_vars,
                       int64_t total, const void* scale_ptrs, const int32_t* scale_len,
                       mtlssl_stream_t stream);
/* Batched refresh of the folded inference-mode BatchNorm constants after an optimizer step moved gamma /
 * beta (slim arg scopes that leave BatchNorm trainable: MobileNet-v1, Inception-ResNet-v2): for every layer l
 * of the six device pointer tables (n_layers device pointers each; gamma[l] may be null = no scale variable)
 *   scale_l[c] = gamma_l[c] * inv_std_l[c]   (only when gamma_l != null)
 *   shift_l[c] = beta_l[c] - mean_l[c] * scale_l[c]
 * for c < channels[l] (device int32 array), one launch for the whole model. */
int mtlssl_bn_refresh(int n_layers, const void* gamma_ptrs, const void* beta_ptrs, const void* mean_ptrs,
                      const void* inv_std_ptrs, const void* scale_ptrs, const void* shift_ptrs,
                      const int32_t* channels, int max_channels, mtlssl_stream_t stream);
/* Elementwise helpers used by the graph glue. */
int mtlssl_axpby(const float* x, float* y, int64_t n, float a, float b, mtlssl_stream_t s); /* y=a*x+b*y */
int mtlssl_scale_channels(const float* w, const float* scale, float* out, int64_t rows, int K,
                          mtlssl_stream_t s); /* out[r,k] = w[r,k]*scale[k] (BN fold) */
int mtlssl_tanh_bwd(const float* y, const float* dy, float* dx, int64_t n, mtlssl_stream_t s);
int mtlssl_relu_bwd(const float* y, const float* dy, float* dx, int64_t n, mtlssl_stream_t s);
/* dx = dy * (0 < y < 6): gradient of tf.nn.relu6 (slim/nets/mobilenet_v1.py:376-413 arg scope). */
int mtlssl_relu6_bwd(const float* y, const float* dy, float* dx, int64_t n, mtlssl_stream_t s);
/* out[r,c] = x[r,c] + bias[c]: channel-mean subtraction of
 * models/faster_rcnn_resnet_v1_feature_extractor.py:74-90 (pass the negated means). */
int mtlssl_bias_add_channels(const float* x, const float* bias, float* out, int64_t rows, int C,
                             mtlssl_stream_t s);
/* out[p,c] = x[p,2-c] - mean[c] for p < npix, c < 3 (mean: 3 device floats, in the OUTPUT's channel order): RGB -> BGR
 * and Caffe's mean subtraction of models/faster_rcnn_vgg_16_feature_extractor.py:43-49 in one pass. One IEEE
 * subtraction per element; out may be x. */
int mtlssl_preprocess_bgr(const float* x, const float* mean, float* out, int64_t npix, mtlssl_stream_t s);
/* tf.one_hot(depth=2) of a 0/1 float vector (faster_rcnn_meta_arch.py:1646-1647). */
int mtlssl_onehot2(const float* t, float* out, int64_t n, mtlssl_stream_t s);

/* ------------------------------------------------------------------ loss-weight glue
 * Per-image normalisers are computed on the device so the step never syncs with the host. */

/* _loss_rpn normalisation (faster_rcnn_meta_arch.py:1644-1659): S_b = sum_i sampled[b,i];
 * loc_scale = sampled*reg_w*loc_coef/S_b; obj_scale = sampled*obj_coef/S_b
 * (coef = loss_weight / batch). */
int mtlssl_rpn_loss_scales(const float* sampled, const float* reg_w, int batch, int n,
                           float loc_coef, float obj_coef, float* loc_scale_out,
                           float* obj_scale_out, mtlssl_stream_t stream);
/* _loss_box_classifier normalisation (faster_rcnn_meta_arch.py:1715-1725,1774-1789):
 * normalizer = max(1,num_proposals[b])*batch; pad = i < num_proposals[b];
 * cls_scale = cls_w*pad/normalizer*cls_coef; loc_scale = reg_w*pad/normalizer*loc_coef;
 * clo_scale (nullable) = reg_w/max(1,sum_i reg_w[b,i]) * sum_{k>=1} closeness_targets[b,i,k] * clo_coef. */
int mtlssl_detector_loss_scales(const float* cls_w, const float* reg_w, const int32_t* num_proposals,
                                const float* closeness_targets, int batch, int n2, int k1,
                                float cls_coef, float loc_coef, float clo_coef, float* cls_scale_out,
                                float* loc_scale_out, float* clo_scale_out, mtlssl_stream_t stream);
/* Second-stage localisation loss (faster_rcnn_meta_arch.py:1735-1749): pick, per proposal, the
 * box encoding of its target class (background slot = zeros) and apply smooth-L1.
 * refined [rows,K,4]; cls_targets [rows,K+1]; d_refined is zero-filled then written. */
int mtlssl_box_select_smooth_l1(const float* refined, const float* cls_targets,
                                const float* reg_targets, const float* row_scale, int rows, int K,
                                float sigma, float* row_loss_out, float* d_refined_out,
                                mtlssl_stream_t stream);
/* _loss_edgemask target preparation (faster_rcnn_meta_arch.py:1862-1868):
 * gt [B,2,H,W] (fg, weight) -> targets [B,H,W,2] = (1-fg, fg), row_scale = weight*coef. */
int mtlssl_edgemask_targets(const float* gt, int batch, int H, int W, float coef,
                            float* targets_out, float* row_scale_out, mtlssl_stream_t stream);
/* predict_with_mtl_results window expansion (faster_rcnn_meta_arch.py:774-803):
 * out [B,n_expand,n2,4], window i = proposal pushed i/(n_expand-1) of the way to the image. */
int mtlssl_expand_windows(const float* proposals_norm, int batch, int n2, int n_expand, float* out,
                          mtlssl_stream_t stream);
/* Exact de-duplication of the refiner's expanded windows [B,n_expand,n2,4] (faster_rcnn_meta_arch.py:774-803):
 * window n_expand-1 of every proposal is the proposal pushed all the way to the full image — [0,0,1,1] up to
 * the last bit of the fp32 sum z + (1 - z) — so that group holds only a handful of DISTINCT boxes per image,
 * which the reference nevertheless crops and runs through the window tower once per proposal. rois_out
 * [B,(n_expand-1)*n2+capacity,4] = windows 0..n_expand-2 unchanged, then the distinct boxes of the last group
 * (bitwise comparison, first-occurrence order, unused slots repeat the first); src_row int32 [B,n_expand,n2] =
 * the row of rois_out (flattened over B) that holds each window, i.e. the gather that expands the tower's
 * outputs back to [B,n_expand,n2]. *overflow (device int32, zeroed by the caller) is set to 1 if an image has
 * more than `capacity` distinct last windows (then results are wrong and the caller must fail). */
int mtlssl_dedup_windows(const float* windows, int batch, int n_expand, int n2, int capacity, float* rois_out,
                         int32_t* src_row, int32_t* overflow, mtlssl_stream_t stream);
/* core/losses.py:418-631 HardExampleMiner as the second stage applies it (faster_rcnn_meta_arch.py:1758-1762,
 * 1902-1946; builders/losses_builder.py:57-93): per image, tf.image.non_max_suppression over the proposal boxes scored
 * by their per-proposal loss keeps at most num_hard_examples proposals; the loss terms are the sums over the kept
 * ones and only they are back-propagated.
 *   _scores: scores[B,n2] = cls + loc row losses (loss_type 0 BOTH — the row losses carry weight / normaliser),
 *            cls only (1) or loc only (2); rows >= num_proposals[b] get -FLT_MAX, whatever their losses hold: still
 *            candidates, sorted behind every real proposal (mtlssl_nms leaves the sorted slots of -inf scores
 *            unwritten but scans them). Feed each image's row to mtlssl_nms.
 *   _apply:  selected[B,max_selected] / num_selected[B] = the NMS output per image; selected indices >=
 *            num_proposals[b] (padding rows the NMS appended after every real candidate; nullable = none) are
 *            dropped — the reference unpads BEFORE mining (:1921-1929); zeroes the rows of d_box [B*n2, box_ld]
 *            and d_cls [B*n2, cls_ld] that were not kept, writes the mined loss sums per image and, if given,
 *            num_kept_out[b] = how many of selected[b, :] were kept (they lead the row, in mining order). */
int mtlssl_hard_mining_scores(const float* loc_row_loss, const float* cls_row_loss, const int32_t* num_proposals,
                              int batch, int n2, int loss_type, float* scores, mtlssl_stream_t stream);
int mtlssl_hard_mining_apply(const int32_t* selected, const int32_t* num_selected, const int32_t* num_proposals,
                             int batch, int max_selected, int n2, const float* loc_row_loss, const float* cls_row_loss,
                             float* d_box, int box_ld, float* d_cls, int cls_ld, float* loc_loss_out,
                             float* cls_loss_out, int32_t* num_kept_out, mtlssl_stream_t stream);
/* slim.dropout (faster_rcnn_meta_arch.py:838-839 in the refiner's FC stack; core/box_predictor.py:484-488, 590-594 after
 * the predictors' extra FC layers): y[i] = x[i] / keep_prob if element i is kept, else 0. The Bernoulli draw is the
 * samplers' counter hash: kept iff mix32(seed, stream_id, i) < floor(keep_prob * 2^32) — reproducible and identical in
 * the CPU oracle. The backward pass is the same call on the gradient with the same (seed, stream_id). x == y allowed. */
int mtlssl_dropout(const float* x, float* y, int64_t n, float keep_prob, uint32_t seed, uint32_t stream_id,
                   mtlssl_stream_t stream);
/* Refiner input (faster_rcnn_meta_arch.py:817-831), per image: [cls (k1) | window predictions
 * win[B,n_expand,n2,k1] laid out proposal-major (nullable) | closeness (nullable; per-image mean
 * tiled when global_closeness)] -> out [B*n2, ld]. */
int mtlssl_refine_concat(const float* cls, const float* win, const float* clo, int batch, int n2,
                         int k1, int n_expand, int global_closeness, float* out,
                         mtlssl_stream_t stream);

/* ------------------------------------------------------------------ cross-replica communication
 * Replaces the reference's only cross-replica step — the sum of the clones' gradients on the CPU
 * (slim/deployment/model_deploy.py:414-444 _sum_clones_gradients, :265-307 optimize_clones; the loss of
 * each clone is pre-scaled by 1/num_clones, :221-223) — and its shared-variable placement (one copy of
 * every variable on the CPU read by all towers, :640-675): here one process per GPU holds a replica in
 * HBM, rank 0 broadcasts the initial values and the gradient buckets are summed GPU-to-GPU by RCCL
 * all-reduce over xGMI. Thin wrappers: one communicator rank per process, bound to the device that is
 * current when mtlssl_comm_init is called; collectives are asynchronous on the given stream and in place.
 * Bootstrap: rank 0 calls mtlssl_comm_unique_id and ships the MTLSSL_COMM_ID_BYTES to the other ranks by
 * any host channel (the Python host uses a torch.distributed gloo store), then EVERY rank calls
 * mtlssl_comm_init (collective). RCCL is bound with dlopen at first use; MTLSSL_ECOMM if it is missing. */
#define MTLSSL_COMM_ID_BYTES 128
typedef struct mtlssl_comm* mtlssl_comm_t;
#define MTLSSL_COMM_F32 0
#define MTLSSL_COMM_F64 1
#define MTLSSL_COMM_I32 2
#define MTLSSL_COMM_I64 3
#define MTLSSL_COMM_SUM 0
#define MTLSSL_COMM_MAX 1
#define MTLSSL_COMM_MIN 2
/* Non-collective probe of the preconditions of mtlssl_comm_init on THIS rank: RCCL can be loaded and every entry
 * point is bound (rccl_version_out, nullable) and a HIP device is current and usable (device_out, nullable).
 * MTLSSL_ECOMM with the reason in mtlssl_last_error otherwise. Ranks agree on the result over their host channel
 * BEFORE any of them enters the collective mtlssl_comm_init (a rank that fails alone would leave the others blocked). */
int mtlssl_comm_available(int* rccl_version_out, int* device_out);
int mtlssl_comm_unique_id(void* id_out);
int mtlssl_comm_init(mtlssl_comm_t* comm_out, const void* id, int nranks, int rank);
/* What RCCL itself reports for the communicator (ncclCommCount / UserRank / CuDevice / ncclGetVersion);
 * any output pointer may be null. */
int mtlssl_comm_info(mtlssl_comm_t comm, int* nranks, int* rank, int* device, int* rccl_version);
/* buf[i] = op over ranks of buf[i], count elements of dtype (device memory). */
int mtlssl_comm_allreduce(mtlssl_comm_t comm, void* buf, int64_t count, int dtype, int op,
                          mtlssl_stream_t stream);
/* bytes of buf on every rank = rank root's. */
int mtlssl_comm_broadcast(mtlssl_comm_t comm, void* buf, int64_t bytes, int root, mtlssl_stream_t stream);
int mtlssl_comm_destroy(mtlssl_comm_t comm);
/* Diagnostic (no reference counterpart): `workgroups` workgroups of `threads` threads and `lds_bytes` of LDS that stay
 * resident and issuing for `microseconds` of wall time on `stream` — a stand-in for the CU share a collective's
 * channels take from the compute streams while gradients are reduced under backward (model_deploy.py:414-444 has the
 * clones' gradients summed on the CPU; here RCCL's kernels share the GPU with the step). tools/cu_thief_probe.py. */
int mtlssl_debug_cu_thief(int workgroups, int threads, int lds_bytes, int64_t microseconds, float* sink,
                          mtlssl_stream_t stream);

/* ------------------------------------------------------------------ evaluation-time visualisation
 * Replaces the rectangle part of utils/visualization_utils.py draw_bounding_box_on_image (PIL ImageDraw.line around
 * the box) as eval_util.py:553-672 visualize_detection_results calls it for the first eval_config.num_visualizations
 * images (evaluator.py:289-310): groundtruth boxes underneath, then the detections. Label text stays on the host.
 *   image [height, width, 3] uint8 on the device, rows row_stride BYTES apart (>= 3 * width), painted in place;
 *   boxes [n,4] int32 absolute pixels (ymin, xmin, ymax, xmax), half open: box i covers rows [ymin, ymax) and columns
 *   [xmin, xmax); colors [n,3] uint8 RGB. The outline of box i = its pixels that are NOT inside
 *   [ymin+thickness, ymax-thickness) x [xmin+thickness, xmax-thickness). Boxes are painted in input order (where
 *   outlines overlap the LAST box wins), clipped to the image; a box with ymax <= ymin or xmax <= xmin paints nothing;
 *   pixels that no outline covers are not written. thickness >= 1. */
int mtlssl_draw_boxes(uint8_t* image, int height, int width, int64_t row_stride, const int32_t* boxes,
                      const uint8_t* colors, int n, int thickness, mtlssl_stream_t stream);

/* ------------------------------------------------------------------ training summaries
 * Replaces the variable histograms of object_detection/trainer.py:440-441 (`for model_var in slim.get_model_variables():
 * global_summaries.add(tf.summary.histogram(model_var.op.name, model_var))`): TensorFlow's HistogramSummary op runs
 * histogram::Histogram::Add (tensorflow/core/lib/histogram/histogram.cc) over each variable on the host; here one pass
 * over a flat parameter buffer (ParamStore.weights / .frozen) does it for every variable at once.
 *   buf            the flat fp32 buffer; variable v is buf[offsets[v] .. offsets[v] + sizes[v]) — what lies between two
 *                  variables (alignment padding) is never read into a result. offsets are multiples of 4 floats off a
 *                  16-byte aligned buf (ParamStore aligns them to 64) for the 16-byte loads; others are read by element.
 *   chunk_table    int32 [num_vars + 1 + 2 * num_chunks], built once per buffer by the host: first the index of every
 *                  variable's first chunk and num_chunks at [num_vars] (a variable of size s has
 *                  ceil(s / MTLSSL_HISTOGRAM_CHUNK) consecutive chunks, none when empty), then per chunk the pair
 *                  (variable, chunk index within the variable). One workgroup per chunk.
 *   bucket_limits  double [num_limits], increasing; num_limits <= MTLSSL_HISTOGRAM_MAX_LIMITS (the table and one
 *                  workgroup's uint32 counts live in LDS). A finite x is counted in the first bucket whose limit is
 *                  strictly greater than double(x) (std::upper_bound, compared in double; denormals as themselves), in
 *                  the last one when no limit is.
 *   moments        double [num_vars, 6]: min, max, num, sum (of double(x)), sum_squares (of double(x) * double(x)),
 *                  nonfinite. NaN and +-inf are counted in nonfinite and left out of everything else. An empty variable,
 *                  or one with no finite value, has min = DBL_MAX, max = -DBL_MAX, num = 0.
 *   counts         uint32 [num_vars, num_limits], zeroed by the call.
 *   workspace      mtlssl_variable_histograms_workspace_bytes(num_chunks) bytes (the chunks' moment partials).
 * All pointers are device memory. No floating-point atomics: bins are added with integer atomics and the moments are
 * folded in a fixed order (thread, wave, chunk ascending), so two calls on the same data agree bit for bit. */
#define MTLSSL_HISTOGRAM_CHUNK 16384
#define MTLSSL_HISTOGRAM_MAX_LIMITS 4096
int64_t mtlssl_variable_histograms_workspace_bytes(int num_chunks);
int mtlssl_variable_histograms(const float* buf, const int32_t* offsets, const int32_t* sizes, int num_vars,
                               const int32_t* chunk_table, int num_chunks, const double* bucket_limits, int num_limits,
                               double* moments, uint32_t* counts, void* workspace, int64_t workspace_bytes,
                               mtlssl_stream_t stream);

/* CRC-32C (Castagnoli) of a HOST buffer, continuing from `crc` (0 to start): the checksum of the reference's
 * data containers — TFRecord framing (tensorflow/core/lib/io/record_writer.cc; the create_records scripts write them,
 * builders/input_reader_builder.py:34-65 reads them) and TensorFlow checkpoint tables / tensors
 * (trainer.py:309-356). Plain host code, no GPU work; returns the 32-bit value. */
int64_t mtlssl_crc32c_host(const void* data, int64_t nbytes, int64_t crc);

#ifdef __cplusplus
}
#endif
#endif /* MTLSSL_HIP_H_ */
