// The PASCAL evaluator's tp/fp labelling for every groundtruth subset at once (gfx950): what
// utils/per_image_evaluation.py:233-281 does per image and class, once per subset, as restated on the host by
// PascalDetectionEvaluator._tp_fp with is_difficult = ~member(subset) (mtl_ssl_amd/evaluation.py), which defines the
// semantics. A detection's best-IoU groundtruth box does not depend on the subset: the IoUs and the arg-max are computed
// once per detection by the whole wavefront, and lane s only decides what that box means in subset s. Exact work: the
// IoUs are iou_matrix's double arithmetic operation for operation, everything after them is comparisons and bits.
//
// Built with -ffp-contract=off: (area_a + area_b) - inter and the products around it must round as numpy rounds them.
#include "common.h"

namespace mtlssl {

namespace {

constexpr int PASCAL_THREADS = 64;   // one wavefront per segment: lane s owns subset s

// np.minimum / np.maximum: a NaN operand propagates
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

struct PascalMatchLds {
  double box[MTLSSL_PASCAL_MATCH_MAX_GT][4];     // the segment's groundtruth boxes, input order
  uint64_t member[MTLSSL_PASCAL_MATCH_MAX_GT];   // bit s: the box belongs to subset s
};

// One lane's set of claimed groundtruth boxes: four words in registers, selected without dynamic indexing.
struct ClaimedSet {
  uint64_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
  __device__ __forceinline__ bool has(int g) const {
    const uint64_t w = g < 64 ? w0 : (g < 128 ? w1 : (g < 192 ? w2 : w3));
    return (w >> (g & 63)) & 1;
  }
  __device__ __forceinline__ void add(int g) {
    const uint64_t b = (uint64_t)1 << (g & 63);
    if (g < 64) w0 |= b; else if (g < 128) w1 |= b; else if (g < 192) w2 |= b; else w3 |= b;
  }
};
static_assert(MTLSSL_PASCAL_MATCH_MAX_GT == 256, "ClaimedSet holds four 64-bit words");

// np.argmax's order on (value, index) pairs: the first NaN if there is one, otherwise the first maximum. An index of
// -1 is "no box yet" and loses to everything.
__device__ __forceinline__ bool argmax_before(double v, int i, double w, int j) {
  if (i < 0) return false;
  if (j < 0) return true;
  const bool vn = v != v, wn = w != w;
  if (vn != wn) return vn;
  if (vn || v == w) return i < j;
  return v > w;
}

__global__ void __launch_bounds__(PASCAL_THREADS)
k_pascal_match(const int32_t* __restrict__ dt_off, const int32_t* __restrict__ gt_off,
               const double* __restrict__ dt_boxes, const double* __restrict__ gt_boxes,
               const uint64_t* __restrict__ gt_member, double thr, int num_subsets,
               uint64_t* __restrict__ tp, uint64_t* __restrict__ drop, unsigned char* __restrict__ hit) {
  __shared__ PascalMatchLds L;
  const int seg = blockIdx.x, lane = threadIdx.x;
  const int d0 = dt_off[seg], D = dt_off[seg + 1] - d0;
  const int g0 = gt_off[seg], G = gt_off[seg + 1] - g0;
  if (D <= 0) return;
  if (G < 0 || G > MTLSSL_PASCAL_MATCH_MAX_GT) {   // the host checks the bound; never index LDS past it
    for (int di = lane; di < D; di += PASCAL_THREADS) {
      tp[d0 + di] = 0;
      drop[d0 + di] = 0;
      hit[d0 + di] = MTLSSL_PASCAL_MATCH_LEFT_OUT;
    }
    return;
  }
  for (int g = lane; g < G; g += PASCAL_THREADS) {
    const double* b = gt_boxes + 4 * (int64_t)(g0 + g);
    L.box[g][0] = b[0]; L.box[g][1] = b[1]; L.box[g][2] = b[2]; L.box[g][3] = b[3];
    L.member[g] = gt_member[g0 + g];
  }
  __syncthreads();

  ClaimedSet claimed;
  for (int di = 0; di < D; ++di) {
    const double* d = dt_boxes + 4 * (int64_t)(d0 + di);
    const double dy0 = d[0], dx0 = d[1], dy1 = d[2], dx1 = d[3];
    const double ad = (dy1 - dy0) * (dx1 - dx0);
    // iou_matrix row of this detection, boxes lane, lane + 64, ...: the indices of a lane ascend, so a later box only
    // replaces the lane's best when it comes strictly before it in np.argmax's order
    double best = 0.0;
    int arg = -1;
    for (int g = lane; g < G; g += PASCAL_THREADS) {
      const double ih = np_max(0.0, np_min(dy1, L.box[g][2]) - np_max(dy0, L.box[g][0]));
      const double iw = np_max(0.0, np_min(dx1, L.box[g][3]) - np_max(dx0, L.box[g][1]));
      const double inter = ih * iw;
      const double ag = (L.box[g][2] - L.box[g][0]) * (L.box[g][3] - L.box[g][1]);
      const double iou = inter / ((ad + ag) - inter);
      if (argmax_before(iou, g, best, arg)) { best = iou; arg = g; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                 // xor butterfly: every lane ends with the segment's arg-max
      const double ov = __shfl_xor(best, o, 64);
      const int oi = __shfl_xor(arg, o, 64);
      if (argmax_before(ov, oi, best, arg)) { best = ov; arg = oi; }
    }
    const bool over = arg >= 0 && best >= thr;         // a NaN IoU is never over the threshold
    bool is_tp = false, is_drop = false;
    if (over && lane < num_subsets) {
      if (!((L.member[arg] >> lane) & 1)) {
        is_drop = true;                                // its box is outside the subset: neither true nor false positive
      } else if (!claimed.has(arg)) {
        is_tp = true;
        claimed.add(arg);
      }
    }
    const uint64_t tbits = __ballot(is_tp), dbits = __ballot(is_drop);
    if (lane == 0) {
      tp[d0 + di] = tbits;
      drop[d0 + di] = dbits;
      hit[d0 + di] = over ? 1 : 0;
    }
  }
}

}  // namespace

}  // namespace mtlssl

using namespace mtlssl;

extern "C" int mtlssl_pascal_match(const int32_t* dt_off, const int32_t* gt_off, int num_segments, int max_gt,
                                   const double* dt_boxes, const double* gt_boxes, const uint64_t* gt_member,
                                   double iou_threshold, int num_subsets, uint64_t* tp, uint64_t* drop, uint8_t* hit,
                                   mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(num_segments >= 0, "pascal_match: num_segments %d < 0", num_segments);
  MTLSSL_REQUIRE(num_subsets > 0 && num_subsets <= PASCAL_THREADS,
                 "pascal_match: %d subsets, one wavefront holds at most %d (one lane each)", num_subsets,
                 PASCAL_THREADS);
  MTLSSL_REQUIRE(max_gt >= 0 && max_gt <= MTLSSL_PASCAL_MATCH_MAX_GT,
                 "pascal_match: a class of one image has %d groundtruth boxes, a lane's claimed set holds at most %d "
                 "(evaluate larger segments on the host)", max_gt, MTLSSL_PASCAL_MATCH_MAX_GT);
  if (num_segments == 0) return MTLSSL_OK;
  MTLSSL_REQUIRE(dt_off && gt_off && dt_boxes && tp && drop && hit, "pascal_match: null buffer");
  MTLSSL_REQUIRE(max_gt == 0 || (gt_boxes && gt_member), "pascal_match: null groundtruth buffer");
  hipLaunchKernelGGL(k_pascal_match, dim3(num_segments), dim3(PASCAL_THREADS), 0, S(stream), dt_off, gt_off, dt_boxes,
                     gt_boxes, gt_member, iou_threshold, num_subsets, tp, drop, hit);
  return check_launch("pascal_match");
}
