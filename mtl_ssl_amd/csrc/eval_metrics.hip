// Evaluation-side kernels (gfx950): the evaluator's per-class re-suppression of one image's detections
// (utils/np_box_list_ops.py:185-366 as wired by utils/per_image_evaluation.py:35-68, 258) and the per-pixel work of
// the edge-mask metric (utils/mtl_util.py:91-101).
//
// Built with -ffp-contract=off: the double arithmetic below is the reference's numpy arithmetic operation for
// operation (np_box_ops.iou, the soft-NMS weights, skimage's bilinear sample), so the kept indices, the rescored
// fp32 scores and the agreement counts are bit-exact against a numpy restatement that uses oracle/portable_math.py
// for the Gaussian exponential.
#include "common.h"
#include "portable_math.h"

namespace mtlssl {

namespace {

constexpr int EVAL_NMS_THREADS = 256;
constexpr int EVAL_NMS_WAVES = EVAL_NMS_THREADS / 64;

// np.minimum / np.maximum: a NaN operand propagates
__device__ __forceinline__ double np_min(double a, double b) { return a != a ? a : (b != b ? b : (a < b ? a : b)); }
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// np_box_ops.iou(boxes1=[a], boxes2=[b]) (utils/np_box_ops.py:37-78), one pair
__device__ __forceinline__ double np_iou(const double* a, const double* b) {
  const double ih = np_max(0.0, np_min(a[2], b[2]) - np_max(a[0], b[0]));
  const double iw = np_max(0.0, np_min(a[3], b[3]) - np_max(a[1], b[1]));
  const double inter = ih * iw;
  const double area1 = (a[2] - a[0]) * (a[3] - a[1]);
  const double area2 = (b[2] - b[0]) * (b[3] - b[1]);
  return inter / (area1 + area2 - inter);
}

// Descending order by score; among equal scores the later position first — np.argsort(s, kind="stable")[::-1]
// (sort_by_field's quicksort leaves ties unspecified; the evaluator's scores are distinct in practice).
__device__ __forceinline__ bool before(float sj, int j, float si, int i) { return sj > si || (sj == si && j > i); }

struct EvalNmsLds {
  double box[MTLSSL_EVAL_NMS_MAX_SEGMENT][4];   // boxes in sorted order, double, times the scale
  float score[MTLSSL_EVAL_NMS_MAX_SEGMENT];     // scores in sorted order (rescored in place by soft-NMS)
  int src[MTLSSL_EVAL_NMS_MAX_SEGMENT];         // segment-local input index of each sorted position
  int order[MTLSSL_EVAL_NMS_MAX_SEGMENT];       // output order: sorted positions
  unsigned char valid[MTLSSL_EVAL_NMS_MAX_SEGMENT];
  float red_s[EVAL_NMS_WAVES];
  int red_p[EVAL_NMS_WAVES];
  int m, count, best;
};

// Block-wide "first maximum": the valid position with the largest score > -10, the earliest among equal scores
// (soft_non_max_suppression's inner loop, np_box_list_ops.py:323-329, strict `>` from score_max = -10).
__device__ int block_first_max(EvalNmsLds& L, int m) {
  const int tid = threadIdx.x;
  float bs = -10.0f;
  int bp = -1;
  for (int q = tid; q < m; q += EVAL_NMS_THREADS) {
    const float s = L.score[q];
    if (L.valid[q] && s > bs) { bs = s; bp = q; }   // q increases: a later equal score never replaces
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float os = __shfl_xor(bs, o, 64);
    const int op = __shfl_xor(bp, o, 64);
    if (op >= 0 && (bp < 0 || os > bs || (os == bs && op < bp))) { bs = os; bp = op; }
  }
  if ((tid & 63) == 0) { L.red_s[tid >> 6] = bs; L.red_p[tid >> 6] = bp; }
  __syncthreads();
  if (tid == 0) {
    float s = -10.0f;
    int p = -1;
    for (int w = 0; w < EVAL_NMS_WAVES; ++w) {
      const int op = L.red_p[w];
      if (op >= 0 && (p < 0 || L.red_s[w] > s || (L.red_s[w] == s && op < p))) { s = L.red_s[w]; p = op; }
    }
    L.best = p;
  }
  __syncthreads();
  return L.best;
}

// Ranks the positions [0, n) whose key passes `keep` into L.order (descending score, `before` order); returns how
// many passed. Reads score(i) for i < n.
template <typename Score, typename Keep>
__device__ int block_rank(EvalNmsLds& L, int n, Score score, Keep keep, int* dst) {
  const int tid = threadIdx.x;
  if (tid == 0) L.count = 0;
  __syncthreads();
  for (int i = tid; i < n; i += EVAL_NMS_THREADS) {
    const float si = score(i);
    if (!keep(si)) continue;
    int r = 0;
    for (int j = 0; j < n; ++j) {
      const float sj = score(j);
      r += (keep(sj) && before(sj, j, si, i)) ? 1 : 0;
    }
    dst[r] = i;
    atomicAdd(&L.count, 1);
  }
  __syncthreads();
  return L.count;
}

__global__ void __launch_bounds__(EVAL_NMS_THREADS)
k_eval_nms(const float* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ offsets,
           int nms_type, double iou_threshold, double sigma, double scale_y, double scale_x, int max_output,
           int32_t* __restrict__ index_out, float* __restrict__ scores_out, int32_t* __restrict__ count_out) {
  __shared__ EvalNmsLds L;
  const int seg = blockIdx.x, tid = threadIdx.x;
  const int off = offsets[seg];
  const int n = offsets[seg + 1] - off;
  if (n < 0 || n > MTLSSL_EVAL_NMS_MAX_SEGMENT) {     // the host checks the bound; never index LDS past it
    if (tid == 0) count_out[seg] = -1;
    return;
  }
  const float* sc = scores + off;
  // filter_scores_greater_than(boxlist, -10.0) + sort_by_field(boxlist, 'scores'), then boxes in sorted order
  const int m = block_rank(L, n, [&](int i) { return sc[i]; }, [](float s) { return s > -10.0f; }, L.src);
  for (int p = tid; p < m; p += EVAL_NMS_THREADS) {
    const int i = L.src[p];
    const float* b = boxes + 4 * (int64_t)(off + i);
    L.box[p][0] = (double)b[0] * scale_y;
    L.box[p][1] = (double)b[1] * scale_x;
    L.box[p][2] = (double)b[2] * scale_y;
    L.box[p][3] = (double)b[3] * scale_x;
    L.score[p] = sc[i];
    L.valid[p] = 1;
  }
  __syncthreads();

  int count;
  if (iou_threshold == 1.0) {                         // NMS disabled: sorted and capped (:227-232, :307-312)
    count = m < max_output ? m : max_output;
    for (int k = tid; k < count; k += EVAL_NMS_THREADS) L.order[k] = k;
  } else if (nms_type == MTLSSL_EVAL_NMS_STANDARD) {
    // non_max_suppression :234-257: greedy in sorted order, a box goes when its IoU with a selected one is > thr
    // (the test is `iou <= thr` to stay: a NaN IoU suppresses)
    count = 0;
    for (int p = 0; p < m && count < max_output; ++p) {
      if (!L.valid[p]) continue;                      // uniform: L.valid is only written between the barriers
      if (tid == 0) L.order[count] = p;
      ++count;
      for (int q = p + 1 + tid; q < m; q += EVAL_NMS_THREADS)
        if (L.valid[q] && !(np_iou(L.box[p], L.box[q]) <= iou_threshold)) L.valid[q] = 0;
      __syncthreads();
    }
  } else {
    // soft_non_max_suppression :314-342: pick the first maximum, rescale every remaining valid score by the weight
    // (a double product rounded once to fp32: `scores[valid] = scores[valid] * weight`)
    int selected = 0;
    for (int it = 0; it < m && selected < max_output; ++it) {
      const int b = block_first_max(L, m);
      if (b < 0) break;
      ++selected;
      for (int q = tid; q < m; q += EVAL_NMS_THREADS) {
        if (q == b || !L.valid[q]) continue;
        double iou = np_iou(L.box[b], L.box[q]);
        double w;
        if (nms_type == MTLSSL_EVAL_NMS_SOFT_LINEAR) {
          if (iou < iou_threshold) iou = 0.0;
          w = 1.0 - iou;
        } else {
          w = exp_rn(-(iou * iou) / sigma);
        }
        L.score[q] = (float)((double)L.score[q] * w);
      }
      if (tid == 0) L.valid[b] = 0;
      __syncthreads();
    }
    // filter_scores_greater_than(max(0, -10)) + sort_by_field + cap (:344-349); ties again later position first
    const int kept = block_rank(L, m, [&](int p) { return L.score[p]; }, [](float s) { return s > 0.0f; }, L.order);
    count = kept < max_output ? kept : max_output;
  }
  __syncthreads();
  int32_t* io = index_out + off;
  float* so = scores_out + off;
  for (int k = tid; k < n; k += EVAL_NMS_THREADS) {
    if (k < count) {
      const int p = L.order[k];
      io[k] = L.src[p];
      so[k] = L.score[p];
    } else {
      io[k] = -1;
      so[k] = 0.0f;
    }
  }
  if (tid == 0) count_out[seg] = count;
}

// skimage.transform.resize(x, (h, w, 2)) at order 1 in scikit-image 0.13 / 0.14 (mode='constant', cval=0, no
// anti-aliasing): output pixel (r, c) samples input ((r + 0.5) * Hf / h - 0.5, (c + 0.5) * Wf / w - 0.5) (for a 1x1
// output the same point, the centre), bilinear over the four neighbours, each outside the map read as 0
// (skimage/_shared/interpolation.pxd bilinear_interpolation / get_pixel2d).
__device__ __forceinline__ double em_pixel(const float* x, int Hf, int Wf, long r, long c, int ch) {
  return (r < 0 || r >= Hf || c < 0 || c >= Wf) ? 0.0 : (double)x[((int64_t)r * Wf + c) * 2 + ch];
}

__global__ void __launch_bounds__(256)
k_edgemask_agreement(const float* __restrict__ logits, int Hf, int Wf, const float* __restrict__ gt, int h, int w,
                     int32_t* __restrict__ count) {
  __shared__ int s_wave[4];
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int agree = 0;
  if (idx < (int64_t)h * w) {
    const int r = (int)(idx / w), c = (int)(idx % w);
    const double rin = ((double)r + 0.5) * (double)Hf / (double)h - 0.5;
    const double cin = ((double)c + 0.5) * (double)Wf / (double)w - 0.5;
    const long minr = (long)floor(rin), minc = (long)floor(cin), maxr = (long)ceil(rin), maxc = (long)ceil(cin);
    const double dr = rin - (double)minr, dc = cin - (double)minc;
    float v[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
      const double top = (1.0 - dc) * em_pixel(logits, Hf, Wf, minr, minc, ch) + dc * em_pixel(logits, Hf, Wf, minr, maxc, ch);
      const double bot = (1.0 - dc) * em_pixel(logits, Hf, Wf, maxr, minc, ch) + dc * em_pixel(logits, Hf, Wf, maxr, maxc, ch);
      v[ch] = (float)((1.0 - dr) * top + dr * bot);     // .astype(np.float32)
    }
    const float label = v[0] < v[1] ? 1.0f : 0.0f;
    agree = label == gt[idx] ? 1 : 0;
  }
  agree = wave_sum_i(agree);
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = agree;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(count, s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
}

}  // namespace

}  // namespace mtlssl

using namespace mtlssl;

extern "C" int mtlssl_eval_nms(const float* boxes, const float* scores, const int32_t* segment_offsets,
                               int num_segments, int max_segment, int nms_type, double iou_threshold, double sigma,
                               double scale_y, double scale_x, int max_output, int32_t* index_out, float* scores_out,
                               int32_t* count_out, mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(num_segments >= 0, "eval_nms: num_segments %d < 0", num_segments);
  MTLSSL_REQUIRE(max_segment >= 0 && max_segment <= MTLSSL_EVAL_NMS_MAX_SEGMENT,
                 "eval_nms: a class of one image has %d detections, the evaluator's NMS holds at most %d in LDS "
                 "(a class never has more than post_processing's max_total_detections: lower it)",
                 max_segment, MTLSSL_EVAL_NMS_MAX_SEGMENT);
  MTLSSL_REQUIRE(nms_type == MTLSSL_EVAL_NMS_STANDARD || nms_type == MTLSSL_EVAL_NMS_SOFT_LINEAR ||
                     nms_type == MTLSSL_EVAL_NMS_SOFT_GAUSSIAN,
                 "eval_nms: nms_type %d (1 standard, 2 soft-linear, 3 soft-gaussian)", nms_type);
  MTLSSL_REQUIRE(iou_threshold >= 0.0 && iou_threshold <= 1.0, "eval_nms: IOU threshold must be in [0, 1], got %g",
                 iou_threshold);
  MTLSSL_REQUIRE(max_output >= 0, "eval_nms: max_output_size must be bigger than 0, got %d", max_output);
  if (num_segments == 0) return MTLSSL_OK;
  MTLSSL_REQUIRE(boxes && scores && segment_offsets && index_out && scores_out && count_out,
                 "eval_nms: null buffer");
  hipLaunchKernelGGL(k_eval_nms, dim3(num_segments), dim3(EVAL_NMS_THREADS), 0, S(stream), boxes, scores,
                     segment_offsets, nms_type, iou_threshold, sigma, scale_y, scale_x, max_output, index_out,
                     scores_out, count_out);
  return check_launch("eval_nms");
}

extern "C" int mtlssl_edgemask_agreement(const float* logits, int Hf, int Wf, const float* gt_mask, int h, int w,
                                         int32_t* count_out, mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(Hf > 0 && Wf > 0 && h > 0 && w > 0, "edgemask_agreement: empty map (%dx%d -> %dx%d)", Hf, Wf, h, w);
  MTLSSL_REQUIRE(logits && gt_mask && count_out, "edgemask_agreement: null buffer");
  hipStream_t st = S(stream);
  if (hipMemsetAsync(count_out, 0, sizeof(int32_t), st) != hipSuccess) return check_launch("edgemask_agreement");
  const int64_t px = (int64_t)h * w;
  hipLaunchKernelGGL(k_edgemask_agreement, dim3((unsigned)cdiv(px, 256)), dim3(256), 0, st, logits, Hf, Wf, gt_mask,
                     h, w, count_out);
  return check_launch("edgemask_agreement");
}
