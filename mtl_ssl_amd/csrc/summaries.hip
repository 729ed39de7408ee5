// Training-summary kernels (gfx950): the histogram and moments of every model variable in one pass over a flat
// parameter buffer — what object_detection/trainer.py:440-441 asks of TensorFlow's HistogramSummary op for each
// variable (tensorflow/core/lib/histogram/histogram.cc: Histogram::Add over the default bucket limits).
//
// Built with -ffp-contract=off: every comparison and every sum below is plain double arithmetic on double(x), so the
// bucket counts, min, max and num are bit-exact against a numpy float64 restatement; sum and sum_squares are summed in a
// fixed order (per thread, per wave, per chunk, chunks ascending), so two runs agree bit for bit.
#include <float.h>

#include "common.h"

namespace mtlssl {

namespace {

constexpr int HIST_THREADS = 256;
constexpr int HIST_WAVES = HIST_THREADS / 64;
constexpr int HIST_CHUNK = MTLSSL_HISTOGRAM_CHUNK;
constexpr int HIST_PARTIAL = 6;       // min, max, num, sum, sum_squares, nonfinite

// double(x) from the bit pattern when x is zero or denormal: exact whatever the wave's denormal mode makes of a
// float -> double conversion (a denormal is mantissa * 2^-149)
__device__ __forceinline__ double to_double(float x) {
  const uint32_t bits = __float_as_uint(x);
  if ((bits & 0x7f800000u) != 0u) return (double)x;
  const double m = (double)(int)(bits & 0x007fffffu) * 0x1p-149;
  return (bits >> 31) ? -m : m;
}

struct Moments {
  double mn, mx, num, sum, sq, bad;
};

__device__ __forceinline__ void fold(Moments& a, const Moments& b) {
  a.mn = b.mn < a.mn ? b.mn : a.mn;
  a.mx = b.mx > a.mx ? b.mx : a.mx;
  a.num += b.num;
  a.sum += b.sum;
  a.sq += b.sq;
  a.bad += b.bad;
}

__device__ __forceinline__ double shfl_xor_d(double v, int o) { return __shfl_xor(v, o, 64); }

// One element: non-finite values are only counted; the others go into the first bucket whose limit is strictly
// greater than double(x) (std::upper_bound) and into the moments.
__device__ __forceinline__ void add_value(float xf, const double* limits, uint32_t* hist, int num_limits, Moments& m) {
  const uint32_t bits = __float_as_uint(xf);
  if ((bits & 0x7f800000u) == 0x7f800000u) {          // NaN, +inf, -inf
    m.bad += 1.0;
    return;
  }
  const double x = to_double(xf);
  int lo = 0, hi = num_limits;                         // first index in [0, num_limits] with limits[index] > x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (limits[mid] > x) hi = mid; else lo = mid + 1;
  }
  if (lo >= num_limits) lo = num_limits - 1;           // a table that ends below x (the default one ends at DBL_MAX)
  atomicAdd(&hist[lo], 1u);
  m.mn = x < m.mn ? x : m.mn;
  m.mx = x > m.mx ? x : m.mx;
  m.num += 1.0;
  m.sum += x;
  m.sq += x * x;
}

// One workgroup per chunk of chunk_table (after its num_vars + 1 header): (variable, chunk index within it).
__global__ void __launch_bounds__(HIST_THREADS)
k_variable_histograms(const float* __restrict__ buf, const int32_t* __restrict__ offsets,
                      const int32_t* __restrict__ sizes, int num_vars, const int32_t* __restrict__ chunks,
                      const double* __restrict__ bucket_limits, int num_limits, uint32_t* __restrict__ counts,
                      double* __restrict__ partials) {
  extern __shared__ double lds[];
  double* limits = lds;                                                   // [num_limits]
  uint32_t* hist = reinterpret_cast<uint32_t*>(lds + num_limits);          // [num_limits]
  __shared__ double red[HIST_WAVES][HIST_PARTIAL];
  const int tid = threadIdx.x;
  const int var = chunks[2 * blockIdx.x], k = chunks[2 * blockIdx.x + 1];
  Moments m = {DBL_MAX, -DBL_MAX, 0.0, 0.0, 0.0, 0.0};
  int64_t len = 0;
  const float* src = nullptr;
  if (var >= 0 && var < num_vars && k >= 0) {                              // a malformed table reads nothing
    const int64_t size = sizes[var], start = (int64_t)k * HIST_CHUNK;
    if (start < size) {
      len = size - start < HIST_CHUNK ? size - start : HIST_CHUNK;
      src = buf + (int64_t)offsets[var] + start;
    }
  }
  for (int i = tid; i < num_limits; i += HIST_THREADS) {
    limits[i] = bucket_limits[i];
    hist[i] = 0u;
  }
  __syncthreads();
  if (len > 0) {
    const bool aligned = (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
    const int64_t quads = aligned ? len >> 2 : 0;
    const float4* src4 = reinterpret_cast<const float4*>(src);
    for (int64_t q = tid; q < quads; q += HIST_THREADS) {
      const float4 v = src4[q];
      add_value(v.x, limits, hist, num_limits, m);
      add_value(v.y, limits, hist, num_limits, m);
      add_value(v.z, limits, hist, num_limits, m);
      add_value(v.w, limits, hist, num_limits, m);
    }
    for (int64_t i = quads * 4 + tid; i < len; i += HIST_THREADS) add_value(src[i], limits, hist, num_limits, m);
  }
  // fixed-shape reduction: butterfly inside the wave, then the waves in order
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    Moments t = {shfl_xor_d(m.mn, o), shfl_xor_d(m.mx, o), shfl_xor_d(m.num, o),
                 shfl_xor_d(m.sum, o), shfl_xor_d(m.sq, o), shfl_xor_d(m.bad, o)};
    fold(m, t);
  }
  if ((tid & 63) == 0) {
    double* r = red[tid >> 6];
    r[0] = m.mn; r[1] = m.mx; r[2] = m.num; r[3] = m.sum; r[4] = m.sq; r[5] = m.bad;
  }
  __syncthreads();                                                          // also: every LDS bin is final
  if (tid == 0) {
    Moments a = {red[0][0], red[0][1], red[0][2], red[0][3], red[0][4], red[0][5]};
    for (int w = 1; w < HIST_WAVES; ++w) {
      Moments b = {red[w][0], red[w][1], red[w][2], red[w][3], red[w][4], red[w][5]};
      fold(a, b);
    }
    double* p = partials + (int64_t)blockIdx.x * HIST_PARTIAL;
    p[0] = a.mn; p[1] = a.mx; p[2] = a.num; p[3] = a.sum; p[4] = a.sq; p[5] = a.bad;
  }
  if (len > 0) {
    uint32_t* dst = counts + (int64_t)var * num_limits;
    for (int i = tid; i < num_limits; i += HIST_THREADS) {
      const uint32_t c = hist[i];
      if (c) atomicAdd(&dst[i], c);                                         // integer adds: any order, one result
    }
  }
}

// One thread per variable folds its chunks' partials in chunk order.
__global__ void __launch_bounds__(64)
k_fold_moments(const int32_t* __restrict__ var_chunk_start, int num_vars, int num_chunks,
               const double* __restrict__ partials, double* __restrict__ moments) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_vars) return;
  int c0 = var_chunk_start[v], c1 = var_chunk_start[v + 1];
  c0 = c0 < 0 ? 0 : c0;
  c1 = c1 > num_chunks ? num_chunks : c1;
  Moments a = {DBL_MAX, -DBL_MAX, 0.0, 0.0, 0.0, 0.0};
  for (int c = c0; c < c1; ++c) {
    const double* p = partials + (int64_t)c * HIST_PARTIAL;
    Moments b = {p[0], p[1], p[2], p[3], p[4], p[5]};
    fold(a, b);
  }
  double* o = moments + (int64_t)v * HIST_PARTIAL;
  o[0] = a.mn; o[1] = a.mx; o[2] = a.num; o[3] = a.sum; o[4] = a.sq; o[5] = a.bad;
}

}  // namespace

}  // namespace mtlssl

using namespace mtlssl;

extern "C" int64_t mtlssl_variable_histograms_workspace_bytes(int num_chunks) {
  return (int64_t)(num_chunks > 0 ? num_chunks : 0) * HIST_PARTIAL * (int64_t)sizeof(double);
}

extern "C" int mtlssl_variable_histograms(const float* buf, const int32_t* offsets, const int32_t* sizes, int num_vars,
                                          const int32_t* chunk_table, int num_chunks, const double* bucket_limits,
                                          int num_limits, double* moments, uint32_t* counts, void* workspace,
                                          int64_t workspace_bytes, mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(num_vars >= 0 && num_chunks >= 0, "variable_histograms: num_vars %d, num_chunks %d", num_vars,
                 num_chunks);
  MTLSSL_REQUIRE(num_limits >= 1 && num_limits <= MTLSSL_HISTOGRAM_MAX_LIMITS,
                 "variable_histograms: %d bucket limits, the limit table and the counts of one workgroup hold at most "
                 "%d in LDS", num_limits, MTLSSL_HISTOGRAM_MAX_LIMITS);
  const int64_t need = mtlssl_variable_histograms_workspace_bytes(num_chunks);
  MTLSSL_REQUIRE(workspace_bytes >= need,
                 "variable_histograms: workspace of %lld bytes, %d chunks need %lld "
                 "(mtlssl_variable_histograms_workspace_bytes)", (long long)workspace_bytes, num_chunks,
                 (long long)need);
  if (num_vars == 0) return MTLSSL_OK;
  MTLSSL_REQUIRE(offsets && sizes && chunk_table && bucket_limits && moments && counts,
                 "variable_histograms: null buffer");
  MTLSSL_REQUIRE(num_chunks == 0 || (buf && workspace), "variable_histograms: null buffer");
  hipStream_t st = S(stream);
  if (hipMemsetAsync(counts, 0, (size_t)num_vars * num_limits * sizeof(uint32_t), st) != hipSuccess)
    return check_launch("variable_histograms");
  double* partials = static_cast<double*>(workspace);
  if (num_chunks > 0) {
    const size_t lds = (size_t)num_limits * (sizeof(double) + sizeof(uint32_t));
    hipLaunchKernelGGL(k_variable_histograms, dim3(num_chunks), dim3(HIST_THREADS), lds, st, buf, offsets, sizes,
                       num_vars, chunk_table + num_vars + 1, bucket_limits, num_limits, counts, partials);
    if (int rc = check_launch("variable_histograms")) return rc;
  }
  hipLaunchKernelGGL(k_fold_moments, dim3((unsigned)cdiv(num_vars, 64)), dim3(64), 0, st, chunk_table, num_vars,
                     num_chunks, partials, moments);
  return check_launch("variable_histograms");
}
