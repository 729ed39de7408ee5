// The MS-COCO evaluator's greedy detection-to-groundtruth match (gfx950): what pycocotools' COCOeval.evaluateImg does per
// (image, category, area range, maxDets), as restated on the host by CocoDetectionEvaluator._iou / _evaluate_image
// (mtl_ssl_amd/evaluation.py), which define the semantics. Exact work: the IoUs are the host's double arithmetic
// operation for operation, everything after them is comparisons and bits.
//
// Built with -ffp-contract=off: (ad + ag) - inter and the products around it must round as numpy rounds them.
#include "common.h"

namespace mtlssl {

namespace {

constexpr int COCO_THREADS = 64;     // one wavefront per segment: lane t*A + a owns threshold t in area range a

// np.minimum / np.maximum: a NaN operand propagates
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

struct CocoMatchLds {
  double box[MTLSSL_COCO_MATCH_MAX_GT][4];    // the segment's groundtruth boxes, input order
  double area[MTLSSL_COCO_MATCH_MAX_GT];
  double iou[MTLSSL_COCO_MATCH_MAX_GT];       // IoUs of the detection at hand against every groundtruth box
  unsigned char crowd[MTLSSL_COCO_MATCH_MAX_GT];
};

// One lane's set of claimed groundtruth boxes: four words in registers, selected without dynamic indexing.
struct GtSet {
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
static_assert(MTLSSL_COCO_MATCH_MAX_GT == 256, "GtSet holds four 64-bit words");

__global__ void __launch_bounds__(COCO_THREADS)
k_coco_match(const int32_t* __restrict__ dt_off, const int32_t* __restrict__ gt_off,
             const double* __restrict__ dt_boxes, const double* __restrict__ gt_boxes,
             const double* __restrict__ gt_area, const unsigned char* __restrict__ gt_crowd,
             const double* __restrict__ iou_thrs, const double* __restrict__ area_rng, int T, int A,
             uint64_t* __restrict__ dt_match, uint64_t* __restrict__ dt_ignore, int32_t* __restrict__ npig) {
  __shared__ CocoMatchLds L;
  const int seg = blockIdx.x, lane = threadIdx.x;
  const int d0 = dt_off[seg], D = dt_off[seg + 1] - d0;
  const int g0 = gt_off[seg], G = gt_off[seg + 1] - g0;
  if (G < 0 || G > MTLSSL_COCO_MATCH_MAX_GT || D < 0) {   // the host checks the bound; never index LDS past it
    if (lane < A) npig[(int64_t)seg * A + lane] = -1;
    return;
  }
  for (int g = lane; g < G; g += COCO_THREADS) {
    const double* b = gt_boxes + 4 * (int64_t)(g0 + g);
    L.box[g][0] = b[0]; L.box[g][1] = b[1]; L.box[g][2] = b[2]; L.box[g][3] = b[3];
    L.area[g] = gt_area[g0 + g];
    L.crowd[g] = gt_crowd[g0 + g] ? 1 : 0;
  }
  __syncthreads();

  // gig of _evaluate_image for one area range: crowd, or the groundtruth area outside [lo, hi] (strict on both sides)
  auto ignored = [&](int g, double lo, double hi) { return L.crowd[g] || L.area[g] < lo || L.area[g] > hi; };

  if (lane < A) {
    const double lo = area_rng[2 * lane], hi = area_rng[2 * lane + 1];
    int n = 0;
    for (int g = 0; g < G; ++g) n += ignored(g, lo, hi) ? 0 : 1;
    npig[(int64_t)seg * A + lane] = n;
  }

  const bool active = lane < T * A;
  const int t = active ? lane / A : 0, a = active ? lane % A : 0;
  const double thr = iou_thrs[t], lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
  const double cap = 1.0 - 1e-10;
  GtSet claimed;
  for (int di = 0; di < D; ++di) {
    const double* d = dt_boxes + 4 * (int64_t)(d0 + di);
    const double dy0 = d[0], dx0 = d[1], dy1 = d[2], dx1 = d[3];
    const double ad = (dy1 - dy0) * (dx1 - dx0);
    __syncthreads();                                   // every lane is done with the previous detection's IoUs
    for (int g = lane; g < G; g += COCO_THREADS) {     // _iou: crowd boxes divide by the detection's area
      const double ih = np_max(0.0, np_min(dy1, L.box[g][2]) - np_max(dy0, L.box[g][0]));
      const double iw = np_max(0.0, np_min(dx1, L.box[g][3]) - np_max(dx0, L.box[g][1]));
      const double inter = ih * iw;
      const double ag = (L.box[g][2] - L.box[g][0]) * (L.box[g][3] - L.box[g][1]);
      const double uni = L.crowd[g] ? ad : ad + ag - inter;
      L.iou[g] = inter / np_max(uni, 1e-300);
    }
    __syncthreads();
    bool dtm = false, dig = false;
    if (active) {
      // The stable sort by gig is two passes over the input order: regular boxes, then ignored ones. With a regular
      // match in hand the host loop breaks at the first ignored box it looks at and no earlier box can still change
      // the match: the second pass is skipped as a whole.
      double best = thr < cap ? thr : cap;
      int m = -1;
      for (int g = 0; g < G; ++g) {
        if (ignored(g, lo, hi)) continue;
        if (claimed.has(g)) continue;                  // a regular box is never crowd: claimed once
        if (L.iou[g] < best) continue;
        best = L.iou[g];                               // an equal IoU replaces the earlier match
        m = g;
      }
      bool m_ignored = false;
      if (m < 0) {
        for (int g = 0; g < G; ++g) {
          if (!ignored(g, lo, hi)) continue;
          if (claimed.has(g) && !L.crowd[g]) continue;
          if (L.iou[g] < best) continue;
          best = L.iou[g];
          m = g;
        }
        m_ignored = true;
      }
      if (m >= 0) {
        dtm = true;
        dig = m_ignored;
        claimed.add(m);
      } else {
        dig = ad < lo || ad > hi;                      // unmatched, and its own area outside the range
      }
    }
    const uint64_t mbits = __ballot(dtm), ibits = __ballot(dig);
    if (lane == 0) {
      dt_match[d0 + di] = mbits;
      dt_ignore[d0 + di] = ibits;
    }
  }
}

}  // namespace

}  // namespace mtlssl

using namespace mtlssl;

extern "C" int mtlssl_coco_match(const int32_t* dt_off, const int32_t* gt_off, int num_segments, int max_gt,
                                 const double* dt_boxes, const double* gt_boxes, const double* gt_area,
                                 const uint8_t* gt_crowd, const double* iou_thrs, int num_iou_thrs,
                                 const double* area_rng, int num_area_rng, uint64_t* dt_match, uint64_t* dt_ignore,
                                 int32_t* npig, mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(num_segments >= 0, "coco_match: num_segments %d < 0", num_segments);
  MTLSSL_REQUIRE(num_iou_thrs > 0 && num_area_rng > 0 && (int64_t)num_iou_thrs * num_area_rng <= COCO_THREADS,
                 "coco_match: %d IoU thresholds x %d area ranges, one wavefront holds at most %d (threshold, range) "
                 "pairs", num_iou_thrs, num_area_rng, COCO_THREADS);
  MTLSSL_REQUIRE(max_gt >= 0 && max_gt <= MTLSSL_COCO_MATCH_MAX_GT,
                 "coco_match: a category of one image has %d groundtruth boxes, a lane's matched set holds at most %d "
                 "(evaluate larger segments on the host)", max_gt, MTLSSL_COCO_MATCH_MAX_GT);
  if (num_segments == 0) return MTLSSL_OK;
  MTLSSL_REQUIRE(dt_off && gt_off && iou_thrs && area_rng && npig, "coco_match: null buffer");
  hipLaunchKernelGGL(k_coco_match, dim3(num_segments), dim3(COCO_THREADS), 0, S(stream), dt_off, gt_off, dt_boxes,
                     gt_boxes, gt_area, gt_crowd, iou_thrs, area_rng, num_iou_thrs, num_area_rng, dt_match, dt_ignore,
                     npig);
  return check_launch("coco_match");
}
