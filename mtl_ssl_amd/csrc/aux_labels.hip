// Auxiliary-task labels made on the device from an image's groundtruth boxes and classes alone (gfx950): the random
// windows and their soft labels, the closeness labels and the edge mask that the reference freezes into its records
// when it writes them (object_detection/create_records/create_pascal_tf_record.py:120-421). The host definitions are
// mtl_ssl_amd/labels.py draw_windows / window_labels_exact / closeness_labels_exact / edgemask_exact.
//
// Built with -ffp-contract=off: the double arithmetic below is the host definitions' arithmetic operation for
// operation, so the windows are bit-exact and the labels differ from the host's only by the order of a sum of
// positive terms. No float atomics: every reduction has a fixed order, outputs are the same bits run to run.
#include "common.h"

namespace mtlssl {

namespace {

constexpr int AUX_THREADS = 256;
constexpr int AUX_WAVES = AUX_THREADS / 64;
constexpr uint32_t kWindowStream = 0x57494E44u;       // labels.WINDOW_STREAM

__device__ __forceinline__ uint32_t aux_mix32(uint32_t seed, uint32_t stream, uint32_t i) {   // glue.hip glue_mix32
  uint32_t x = i + 0x9E3779B9u * seed + 0x85EBCA6Bu * stream;
  x ^= x >> 16; x *= 0x7FEB352Du; x ^= x >> 15; x *= 0x846CA68Bu; x ^= x >> 16;
  return x;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int clamp_num(const int32_t* num, int b, int max_gt) {
  const int n = num[b];
  return n < 0 ? 0 : (n > max_gt ? max_gt : n);
}

// Python's max(0.0, x) / min(hi, x): the second operand only when it is strictly beyond the first
__device__ __forceinline__ double py_max0(double x) { return x > 0.0 ? x : 0.0; }
__device__ __forceinline__ double py_min(double hi, double x) { return x < hi ? x : hi; }

// The class id of every box of image b from the one-hot rows [max_gt, K+1] (column = id, column 0 = background)
__device__ void load_class_ids(const float* __restrict__ classes_bg, int b, int max_gt, int K1, int n, int* cls) {
  for (int g = threadIdx.x; g < n; g += blockDim.x) cls[g] = 0;
  __syncthreads();
  const float* row = classes_bg + (int64_t)b * max_gt * K1;
  for (int e = threadIdx.x; e < n * K1; e += blockDim.x)
    if (row[e] > 0.5f) cls[e / K1] = e % K1;
}

// create_multi_object's random branch (create_pascal_tf_record.py:225-261), one thread per (image, window slot)
__global__ void __launch_bounds__(64)
k_aux_draw_windows(const float* __restrict__ boxes, const int32_t* __restrict__ num, int B, int max_gt, int Wn, double H,
                   double W, double m, uint32_t seed, uint32_t step, uint32_t image0, float* __restrict__ out) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= B * Wn) return;
  const int b = t / Wn, w = t % Wn;
  const int n = clamp_num(num, b, max_gt);
  const float* bx = boxes + (int64_t)b * max_gt * 4;
  const uint32_t s = aux_mix32(aux_mix32(seed, kWindowStream, step), kWindowStream, image0 + (uint32_t)b);
  const uint32_t slot = n ? (uint32_t)w : 0u;                 // an image without boxes repeats its first window
  double ymin = 0.0, xmin = 0.0, ymax = 0.0, xmax = 0.0;
  for (int a = 0; a < MTLSSL_AUX_WINDOW_ATTEMPTS; ++a) {
    const uint32_t c = (slot * MTLSSL_AUX_WINDOW_ATTEMPTS + (uint32_t)a) * 4u;
    const double u0 = (double)(aux_mix32(s, kWindowStream, c) >> 8) * 0x1p-24;
    const double u1 = (double)(aux_mix32(s, kWindowStream, c + 1) >> 8) * 0x1p-24;
    const double u2 = (double)(aux_mix32(s, kWindowStream, c + 2) >> 8) * 0x1p-24;
    const double u3 = (double)(aux_mix32(s, kWindowStream, c + 3) >> 8) * 0x1p-24;
    const double bh = u0 * (H - m) + m, bw = u1 * (W - m) + m;
    const double cy = u2 * H, cx = u3 * W;
    ymin = py_max0(cy - bh / 2);
    xmin = py_max0(cx - bw / 2);
    ymax = py_min(H, cy + bh / 2);
    xmax = py_min(W, cx + bw / 2);
    if (xmax - xmin < m) {
      if (xmin == 0.0) xmax = m;
      else if (xmax == W) xmin = W - m;
    }
    if (ymax - ymin < m) {
      if (ymin == 0.0) ymax = m;
      else if (ymax == H) ymin = H - m;
    }
    bool meets = n == 0;
    for (int g = 0; g < n && !meets; ++g) {
      const double y0 = (double)bx[4 * g] * H, x0 = (double)bx[4 * g + 1] * W;
      const double y1 = (double)bx[4 * g + 2] * H, x1 = (double)bx[4 * g + 3] * W;
      meets = (ymax < y1 ? ymax : y1) > (ymin > y0 ? ymin : y0) && (xmax < x1 ? xmax : x1) > (xmin > x0 ? xmin : x0);
    }
    if (meets) break;
  }
  float* o = out + 4 * (int64_t)t;
  o[0] = (float)(ymin / H);
  o[1] = (float)(xmin / W);
  o[2] = (float)(ymax / H);
  o[3] = (float)(xmax / W);
}

struct WindowLds {
  double box[MTLSSL_AUX_MAX_GT][4];     // boxes clipped to the window, in window units
  double xs[2 * MTLSSL_AUX_MAX_GT];     // their x edges, sorted
  double area[MTLSSL_AUX_MAX_GT + 1];   // union area per class run; slot nrun = all boxes
  int cls[MTLSSL_AUX_MAX_GT];
  int by_y[MTLSSL_AUX_MAX_GT];          // box indices ordered by (ymin, index)
  int by_cls[MTLSSL_AUX_MAX_GT];        // box indices ordered by (class, ymin, index)
  int run[MTLSSL_AUX_MAX_GT + 1];       // where each class's run starts in by_cls
  int nrun;
  double total;
};

// Length of the union of the y intervals of the boxes list[0..len) (ordered by ymin) that span the x slab [a, b]
__device__ __forceinline__ double covered_length(const WindowLds& L, const int* list, int len, double a, double b) {
  double sum = 0.0, lo = 0.0, hi = 0.0;
  bool open = false;
  for (int p = 0; p < len; ++p) {
    const double* bx = L.box[list[p]];
    if (!(bx[1] <= a && bx[3] >= b && bx[2] > bx[0])) continue;
    if (!open || bx[0] > hi) {
      if (open) sum += hi - lo;
      lo = bx[0];
      hi = bx[2];
      open = true;
    } else if (bx[2] > hi) {
      hi = bx[2];
    }
  }
  return open ? sum + (hi - lo) : sum;
}

// get_multi_label (create_pascal_tf_record.py:199-226, label_option 1, normalize_option 1) with get_rect_area_total
// (:140-162) as an exact slab sweep: one workgroup per (image, window), a lane per slab between two consecutive sorted
// x edges, the boxes of a class merged in y in ymin order.
__global__ void __launch_bounds__(AUX_THREADS)
k_aux_window_labels(const float* __restrict__ boxes, const float* __restrict__ classes_bg, const int32_t* __restrict__ num,
                    const float* __restrict__ windows, int max_gt, int K1, int Wn, double H, double W,
                    float* __restrict__ out) {
  __shared__ WindowLds L;
  const int tid = threadIdx.x, b = blockIdx.x / Wn;
  const int n = clamp_num(num, b, max_gt);
  const float* win = windows + 4 * (int64_t)blockIdx.x;
  const double wy0 = (double)win[0] * H, wx0 = (double)win[1] * W, wy1 = (double)win[2] * H, wx1 = (double)win[3] * W;
  const double wh = wy1 - wy0, ww = wx1 - wx0;
  load_class_ids(classes_bg, b, max_gt, K1, n, L.cls);
  for (int g = tid; g < n; g += AUX_THREADS) {
    const float* bx = boxes + ((int64_t)b * max_gt + g) * 4;
    L.box[g][0] = (fmin(fmax((double)bx[0] * H, wy0), wy1) - wy0) / wh;
    L.box[g][1] = (fmin(fmax((double)bx[1] * W, wx0), wx1) - wx0) / ww;
    L.box[g][2] = (fmin(fmax((double)bx[2] * H, wy0), wy1) - wy0) / wh;
    L.box[g][3] = (fmin(fmax((double)bx[3] * W, wx0), wx1) - wx0) / ww;
  }
  for (int e = tid; e < 2 * n; e += AUX_THREADS) L.xs[e] = 0.0;      // a NaN coordinate leaves ranks unused
  for (int g = tid; g < n; g += AUX_THREADS) L.by_y[g] = L.by_cls[g] = g;
  __syncthreads();
  // rank sorts (n <= 256: every thread counts who comes before its element)
  for (int e = tid; e < 2 * n; e += AUX_THREADS) {
    const double v = L.box[e >> 1][1 + 2 * (e & 1)];
    int r = 0;
    for (int f = 0; f < 2 * n; ++f) {
      const double vf = L.box[f >> 1][1 + 2 * (f & 1)];
      r += (vf < v || (vf == v && f < e)) ? 1 : 0;
    }
    L.xs[r] = v;
    if (e < n) {
      const double y = L.box[e][0];
      const int c = L.cls[e];
      int ry = 0, rc = 0;
      for (int f = 0; f < n; ++f) {
        const double yf = L.box[f][0];
        const int cf = L.cls[f];
        const bool y_before = yf < y || (yf == y && f < e);
        ry += y_before ? 1 : 0;
        rc += (cf < c || (cf == c && y_before)) ? 1 : 0;
      }
      L.by_y[ry] = e;
      L.by_cls[rc] = e;
    }
  }
  __syncthreads();
  if (tid == 0) {
    int nrun = 0;
    for (int p = 0; p < n; ++p)
      if (p == 0 || L.cls[L.by_cls[p]] != L.cls[L.by_cls[p - 1]]) L.run[nrun++] = p;
    L.run[nrun] = n;
    L.nrun = nrun;
  }
  __syncthreads();
  const int nrun = L.nrun, wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r <= nrun; r += AUX_WAVES) {             // r == nrun: all boxes (the background slot)
    const int* list = r < nrun ? L.by_cls + L.run[r] : L.by_y;
    const int len = r < nrun ? L.run[r + 1] - L.run[r] : n;
    double acc = 0.0;
    for (int s = lane; s < 2 * n - 1; s += 64) {
      const double a = L.xs[s], bb = L.xs[s + 1];
      if (bb > a) acc += (bb - a) * covered_length(L, list, len, a, bb);
    }
    acc = wave_sum_d(acc);
    if (lane == 0) L.area[r] = acc;
  }
  __syncthreads();
  // sqrt of the area fractions, divided by their sum
  for (int r = tid; r <= nrun; r += AUX_THREADS) L.area[r] = sqrt(r < nrun ? L.area[r] : fmax(0.0, 1.0 - L.area[r]));
  float* o = out + (int64_t)blockIdx.x * K1;
  for (int k = tid; k < K1; k += AUX_THREADS) o[k] = 0.0f;
  __syncthreads();
  if (tid == 0) {
    double total = L.area[nrun];
    for (int r = 0; r < nrun; ++r) total += L.area[r];
    L.total = total;
  }
  __syncthreads();
  const double total = L.total;
  if (tid == 0) o[0] = (float)(L.area[nrun] / total);
  for (int r = tid; r < nrun; r += AUX_THREADS) {
    const int c = L.cls[L.by_cls[L.run[r]]];
    if (c > 0) o[c] = (float)(L.area[r] / total);
  }
}

struct ClosenessLds {
  double cy[MTLSSL_AUX_MAX_GT], cx[MTLSSL_AUX_MAX_GT];
  int cls[MTLSSL_AUX_MAX_GT];
};

// closeness of object i to class c: 1 - (distance to c's nearest centre) / diagonal over the objects of another class
__device__ __forceinline__ double closeness_to(const ClosenessLds& L, int n, int i, int c, double diag) {
  double best = 0.0;
  const int ci = L.cls[i];
  if (c == ci) return best;
  for (int j = 0; j < n; ++j) {
    if (L.cls[j] != c) continue;
    const double dx = L.cx[i] - L.cx[j], dy = L.cy[i] - L.cy[j];
    const double v = 1.0 - sqrt(dx * dx + dy * dy) / diag;
    if (v > best) best = v;
  }
  return best;
}

// get_closeness (create_pascal_tf_record.py:325-358): one wave per (image, object) row
__global__ void __launch_bounds__(64)
k_aux_closeness(const float* __restrict__ boxes, const float* __restrict__ classes_bg, const int32_t* __restrict__ num,
                int max_gt, int K1, double H, double W, float* __restrict__ out) {
  __shared__ ClosenessLds L;
  const int lane = threadIdx.x, b = blockIdx.x / max_gt, i = blockIdx.x % max_gt;
  const int n = clamp_num(num, b, max_gt);
  float* o = out + (int64_t)blockIdx.x * K1;
  if (i >= n) {                                             // uniform over the workgroup
    for (int k = lane; k < K1; k += 64) o[k] = 0.0f;
    return;
  }
  load_class_ids(classes_bg, b, max_gt, K1, n, L.cls);
  for (int g = lane; g < n; g += 64) {
    const float* bx = boxes + ((int64_t)b * max_gt + g) * 4;
    L.cy[g] = ((double)bx[0] * H + (double)bx[2] * H) / 2;
    L.cx[g] = ((double)bx[1] * W + (double)bx[3] * W) / 2;
  }
  __syncthreads();
  const double diag = sqrt(W * W + H * H);
  double rest = 0.0;
  for (int k = lane ? lane : 64; k < K1; k += 64) rest += closeness_to(L, n, i, k, diag);
  rest = wave_sum_d(rest);
  double v0 = closeness_to(L, n, i, 0, diag);
  if (rest == 0.0) v0 = 1.0;                                // nothing of another class around (or a single object)
  const double total = v0 + rest;
  for (int k = lane; k < K1; k += 64) o[k] = (float)((k ? closeness_to(L, n, i, k, diag) : v0) / total);
}

struct EdgemaskLds {
  int y0[MTLSSL_AUX_MAX_GT], x0[MTLSSL_AUX_MAX_GT], y1[MTLSSL_AUX_MAX_GT], x1[MTLSSL_AUX_MAX_GT];
  float weight[MTLSSL_AUX_MAX_GT];
  double part[AUX_WAVES];
};

__device__ __forceinline__ int py_int(double v) {          // int(): towards zero; a wild value must not overflow the cast
  return (int)(v > 1e9 ? 1e9 : (v < -1e9 ? -1e9 : v));
}

// create_edgemask (create_pascal_tf_record.py:375-421): one workgroup per image
__global__ void __launch_bounds__(AUX_THREADS)
k_aux_edgemask(const float* __restrict__ boxes, const int32_t* __restrict__ num, int max_gt, double H, double W, int M,
               float* __restrict__ out) {
  __shared__ EdgemaskLds L;
  const int tid = threadIdx.x, b = blockIdx.x;
  const int n = clamp_num(num, b, max_gt);
  for (int g = tid; g < n; g += AUX_THREADS) {
    const float* bx = boxes + ((int64_t)b * max_gt + g) * 4;
    int y0 = py_int((double)bx[0] * H / H * M);
    int x0 = py_int((double)bx[1] * W / W * M);
    int y1 = py_int((double)bx[2] * H / H * M + 0.99);
    int x1 = py_int((double)bx[3] * W / W * M + 0.99);
    y1 = y1 < M - 1 ? y1 : M - 1;
    x1 = x1 < M - 1 ? x1 : M - 1;
    int bw = x1 - x0 + 1, bh = y1 - y0 + 1;
    if (bw == 0) {
      if (x0 + x1 > M) x0 -= 1; else x1 += 1;
      bw = 1;
    }
    if (bh == 0) {
      if (y0 + y1 > M) y0 -= 1; else y1 += 1;
      bh = 1;
    }
    if (bw < 0 || bh < 0) { y0 = x0 = 0; y1 = x1 = -1; bw = bh = 1; }     // not a box (xmax < xmin): covers nothing
    L.y0[g] = y0; L.x0[g] = x0; L.y1[g] = y1; L.x1[g] = x1;
    L.weight[g] = 1.0f / (float)bw / (float)bh;
  }
  __syncthreads();
  const int cells = M * M;
  float* fg = out + (int64_t)b * 2 * cells;
  float* wt = fg + cells;
  const float base = 1.0f / (float)M / (float)M;
  double sum = 0.0;
  for (int idx = tid; idx < cells; idx += AUX_THREADS) {
    const int r = idx / M, c = idx % M;
    float w = base, m = 0.0f;
    for (int g = 0; g < n; ++g)
      if (r >= L.y0[g] && r <= L.y1[g] && c >= L.x0[g] && c <= L.x1[g]) {
        m = 1.0f;
        w = fmaxf(w, L.weight[g]);
      }
    fg[idx] = m;
    wt[idx] = w;
    sum += (double)w;
  }
  sum = wave_sum_d(sum);
  if ((tid & 63) == 0) L.part[tid >> 6] = sum;
  __syncthreads();
  const float mean = (float)((((L.part[0] + L.part[1]) + L.part[2]) + L.part[3]) / (double)cells);
  for (int idx = tid; idx < cells; idx += AUX_THREADS) wt[idx] = wt[idx] / mean;     // each thread re-reads its own cells
}

}  // namespace

}  // namespace mtlssl

using namespace mtlssl;

#define AUX_REQUIRE_GT(what)                                                                                     \
  MTLSSL_REQUIRE(max_gt >= 1 && max_gt <= MTLSSL_AUX_MAX_GT,                                                     \
                 what ": %d groundtruth rows per image, the label kernels hold at most %d in LDS", max_gt,       \
                 MTLSSL_AUX_MAX_GT)

extern "C" int mtlssl_aux_draw_windows(const float* boxes_norm, const int32_t* num, int batch, int max_gt,
                                       int num_windows, double height, double width, double min_obj_size,
                                       uint32_t seed, uint32_t step, uint32_t image0, float* window_boxes,
                                       mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(batch >= 0 && num_windows >= 0 && max_gt >= 1, "aux_draw_windows: batch %d, windows %d, max_gt %d",
                 batch, num_windows, max_gt);
  MTLSSL_REQUIRE(height > 0.0 && width > 0.0 && min_obj_size >= 0.0, "aux_draw_windows: image %g x %g, min_obj_size %g",
                 height, width, min_obj_size);
  MTLSSL_REQUIRE((int64_t)num_windows * MTLSSL_AUX_WINDOW_ATTEMPTS * 4 < ((int64_t)1 << 32),
                 "aux_draw_windows: %d windows overflow the 32-bit draw counter", num_windows);
  const int64_t total = (int64_t)batch * num_windows;
  if (total == 0) return MTLSSL_OK;
  MTLSSL_REQUIRE(boxes_norm && num && window_boxes, "aux_draw_windows: null buffer");
  hipLaunchKernelGGL(k_aux_draw_windows, dim3((unsigned)cdiv(total, 64)), dim3(64), 0, S(stream), boxes_norm, num,
                     batch, max_gt, num_windows, height, width, min_obj_size, seed, step, image0, window_boxes);
  return check_launch("aux_draw_windows");
}

extern "C" int mtlssl_aux_window_labels(const float* boxes_norm, const float* classes_bg, const int32_t* num,
                                        const float* window_boxes, int batch, int max_gt, int num_classes,
                                        int num_windows, double height, double width, float* labels_out,
                                        mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(batch >= 0 && num_windows >= 0 && num_classes >= 1, "aux_window_labels: batch %d, windows %d, classes %d",
                 batch, num_windows, num_classes);
  AUX_REQUIRE_GT("aux_window_labels");
  MTLSSL_REQUIRE(height > 0.0 && width > 0.0, "aux_window_labels: image %g x %g", height, width);
  if ((int64_t)batch * num_windows == 0) return MTLSSL_OK;
  MTLSSL_REQUIRE(boxes_norm && classes_bg && num && window_boxes && labels_out, "aux_window_labels: null buffer");
  hipLaunchKernelGGL(k_aux_window_labels, dim3((unsigned)(batch * num_windows)), dim3(AUX_THREADS), 0, S(stream),
                     boxes_norm, classes_bg, num, window_boxes, max_gt, num_classes + 1, num_windows, height, width,
                     labels_out);
  return check_launch("aux_window_labels");
}

extern "C" int mtlssl_aux_closeness(const float* boxes_norm, const float* classes_bg, const int32_t* num, int batch,
                                    int max_gt, int num_classes, double height, double width, float* closeness_out,
                                    mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(batch >= 0 && num_classes >= 1, "aux_closeness: batch %d, classes %d", batch, num_classes);
  AUX_REQUIRE_GT("aux_closeness");
  MTLSSL_REQUIRE(height > 0.0 && width > 0.0, "aux_closeness: image %g x %g", height, width);
  if (batch == 0) return MTLSSL_OK;
  MTLSSL_REQUIRE(boxes_norm && classes_bg && num && closeness_out, "aux_closeness: null buffer");
  hipLaunchKernelGGL(k_aux_closeness, dim3((unsigned)(batch * max_gt)), dim3(64), 0, S(stream), boxes_norm, classes_bg,
                     num, max_gt, num_classes + 1, height, width, closeness_out);
  return check_launch("aux_closeness");
}

extern "C" int mtlssl_aux_edgemask(const float* boxes_norm, const int32_t* num, int batch, int max_gt, double height,
                                   double width, int mask_size, float* edgemask_out, mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(batch >= 0 && mask_size >= 1 && mask_size <= 1024, "aux_edgemask: batch %d, mask size %d (1..1024)",
                 batch, mask_size);
  AUX_REQUIRE_GT("aux_edgemask");
  MTLSSL_REQUIRE(height > 0.0 && width > 0.0, "aux_edgemask: image %g x %g", height, width);
  if (batch == 0) return MTLSSL_OK;
  MTLSSL_REQUIRE(boxes_norm && num && edgemask_out, "aux_edgemask: null buffer");
  hipLaunchKernelGGL(k_aux_edgemask, dim3((unsigned)batch), dim3(AUX_THREADS), 0, S(stream), boxes_norm, num, max_gt,
                     height, width, mask_size, edgemask_out);
  return check_launch("aux_edgemask");
}
