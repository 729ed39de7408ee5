// Batch-statistics BatchNorm (slim.batch_norm in training mode) over x [rows, C] — include/mtlssl_hip.h, "batch-statistics
// BatchNorm". HBM/L2-bound: the forward reads x three times and writes y once, the backward reads x, dy (and y) twice and
// writes dx once; a workgroup's slab (rows x 128 B; 0.6 MB at 4 864 x 512) is small enough for L2 to serve the second
// and third pass (measured times: tools/batch_norm_cost.py).
//
// Launch shape (both kernels): one workgroup of 512 threads owns BN_CH = 32 consecutive channels and walks all rows.
// Thread (tx, ty) = (t & 31, t >> 5): channel c0 + tx, row lanes ty + 16 k (k = 0..3), i.e. 64 row lanes per channel,
// each a serial fp32 sum over rows lane, lane + 64, lane + 128, ... A half wave reads the 32 channels of one row: one
// 128-B line. Reduction of a per-channel sum, in this fixed order:
//   serial run per lane   s(rows) = ceil(rows / 64) terms (s - 1 additions: the first term is added to an exact zero)
//   tree                  d = 6: (a0 + a1) + (a2 + a3) in registers (2 levels), then 16 -> 1 over ty in LDS (4 levels)
// so a sum carries at most s - 1 + d roundings, and one more for the division by n. No atomics, no workspace; the
// result does not depend on the grid or on timing. Built with -ffp-contract=off: every product and sum below is its own
// rounding (the moving-average update is specified as an unfused fp32 sequence), and sqrtf and the divisions are the
// correctly rounded ones (-fhip-fp32-correctly-rounded-divide-sqrt, hipcc's default, stated in build.py).
// A channel past C (the ragged last slab) and a row past `rows` are never read or written: their threads only take part
// in the barriers.
#include "common.h"
#include "epilogue.h"

namespace mtlssl {

constexpr int BN_CH = 32;        // channels per workgroup
constexpr int BN_TY = 16;        // row lanes per channel that are threads
constexpr int BN_UNROLL = 4;     // row lanes per thread (independent accumulators, loads in flight)
constexpr int BN_THREADS = BN_CH * BN_TY;
constexpr int BN_STEP = BN_TY * BN_UNROLL;   // 64 row lanes

// Sum over the 16 threads of a channel; every thread of the channel returns the total. `lds` holds BN_THREADS floats.
__device__ __forceinline__ float bn_block_sum(float a0, float a1, float a2, float a3, float* lds, int tx, int ty) {
  lds[ty * BN_CH + tx] = (a0 + a1) + (a2 + a3);
#pragma unroll
  for (int o = BN_TY / 2; o > 0; o >>= 1) {
    __syncthreads();
    if (ty < o) lds[ty * BN_CH + tx] += lds[(ty + o) * BN_CH + tx];
  }
  __syncthreads();
  const float total = lds[tx];
  __syncthreads();                 // the next sum overwrites lds
  return total;
}

constexpr int BN_ACTS = MTLSSL_EPI_RELU | MTLSSL_EPI_RELU6;   // what mtlssl_batch_norm_train_fwd admits

__global__ void __launch_bounds__(BN_THREADS)
    k_batch_norm_train_fwd(const float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                           float* __restrict__ y, float* __restrict__ save_mean, float* __restrict__ save_inv_std,
                           float* __restrict__ moving_mean, float* __restrict__ moving_var, int64_t rows, int C,
                           float eps, float f, int epi) {
  __shared__ float lds[BN_THREADS];
  const int tx = threadIdx.x & (BN_CH - 1), ty = threadIdx.x / BN_CH;
  const int c = blockIdx.x * BN_CH + tx;
  const bool live = c < C;
  const float* xc = x + (live ? c : 0);
  const float n = (float)rows;

  float a[BN_UNROLL] = {0.f, 0.f, 0.f, 0.f};
  if (live)
    for (int64_t r0 = ty; r0 < rows; r0 += BN_STEP) {
#pragma unroll
      for (int k = 0; k < BN_UNROLL; ++k) {
        const int64_t r = r0 + k * BN_TY;
        if (r < rows) a[k] += xc[r * C];
      }
    }
  const float mean = bn_block_sum(a[0], a[1], a[2], a[3], lds, tx, ty) / n;

  float q[BN_UNROLL] = {0.f, 0.f, 0.f, 0.f};
  if (live)
    for (int64_t r0 = ty; r0 < rows; r0 += BN_STEP) {
#pragma unroll
      for (int k = 0; k < BN_UNROLL; ++k) {
        const int64_t r = r0 + k * BN_TY;
        if (r < rows) {
          const float dv = xc[r * C] - mean;
          q[k] += dv * dv;
        }
      }
    }
  const float var = bn_block_sum(q[0], q[1], q[2], q[3], lds, tx, ty) / n;
  const float inv_std = 1.0f / sqrtf(var + eps);
  if (!live) return;               // after the last barrier

  if (ty == 0) {
    save_mean[c] = mean;
    save_inv_std[c] = inv_std;
    if (moving_mean != nullptr) {
      const float mm = moving_mean[c], mv = moving_var[c];
      const float nm1 = rows > 1 ? (float)(rows - 1) : 1.0f;
      const float unbiased = (var * n) / nm1;
      moving_mean[c] = mm - (mm - mean) * f;
      moving_var[c] = mv - (mv - unbiased) * f;
    }
  }
  const float gm = gamma != nullptr ? gamma[c] : 1.0f;
  const float bt = beta != nullptr ? beta[c] : 0.0f;
  float* yc = y + c;
  for (int64_t r0 = ty; r0 < rows; r0 += BN_STEP) {
#pragma unroll
    for (int k = 0; k < BN_UNROLL; ++k) {
      const int64_t r = r0 + k * BN_TY;
      if (r < rows) {
        float v = (xc[r * C] - mean) * inv_std;
        if (gamma != nullptr) v = v * gm;
        if (beta != nullptr) v = v + bt;
        yc[r * C] = act_fwd<BN_ACTS>(v, epi);
      }
    }
  }
}

__global__ void __launch_bounds__(BN_THREADS)
    k_batch_norm_train_bwd(const float* __restrict__ x, const float* __restrict__ dy, const float* __restrict__ y,
                           const float* __restrict__ gamma, const float* __restrict__ save_mean,
                           const float* __restrict__ save_inv_std, float* __restrict__ dx, float* __restrict__ dgamma,
                           float* __restrict__ dbeta, int64_t rows, int C, float accum, int mask) {
  __shared__ float lds[BN_THREADS];
  const int tx = threadIdx.x & (BN_CH - 1), ty = threadIdx.x / BN_CH;
  const int c = blockIdx.x * BN_CH + tx;
  const bool live = c < C;
  const int cc = live ? c : 0;
  const float* xc = x + cc;
  const float* gc = dy + cc;
  const float* yc = mask ? y + cc : nullptr;
  const float mean = save_mean[cc], inv_std = save_inv_std[cc];
  const float n = (float)rows;

  auto masked = [&](int64_t i) {
    float g = gc[i];
    if (mask) g = act_mask(g, yc[i], mask);
    return g;
  };

  float a[BN_UNROLL] = {0.f, 0.f, 0.f, 0.f}, b[BN_UNROLL] = {0.f, 0.f, 0.f, 0.f};
  if (live)
    for (int64_t r0 = ty; r0 < rows; r0 += BN_STEP) {
#pragma unroll
      for (int k = 0; k < BN_UNROLL; ++k) {
        const int64_t r = r0 + k * BN_TY;
        if (r < rows) {
          const float g = masked(r * C);
          const float xh = (xc[r * C] - mean) * inv_std;
          a[k] += g;
          b[k] += g * xh;
        }
      }
    }
  const float sg = bn_block_sum(a[0], a[1], a[2], a[3], lds, tx, ty);
  const float sgx = bn_block_sum(b[0], b[1], b[2], b[3], lds, tx, ty);
  if (!live) return;               // after the last barrier

  if (ty == 0) {
    if (dbeta != nullptr) dbeta[c] = accum != 0.f ? accum * dbeta[c] + sg : sg;
    if (dgamma != nullptr) dgamma[c] = accum != 0.f ? accum * dgamma[c] + sgx : sgx;
  }
  const float kf = gamma != nullptr ? gamma[c] * inv_std : inv_std;
  const float sg_n = sg / n, sgx_n = sgx / n;
  float* dxc = dx + c;
  for (int64_t r0 = ty; r0 < rows; r0 += BN_STEP) {
#pragma unroll
    for (int k = 0; k < BN_UNROLL; ++k) {
      const int64_t r = r0 + k * BN_TY;
      if (r < rows) {
        const float g = masked(r * C);
        const float xh = (xc[r * C] - mean) * inv_std;
        dxc[r * C] = kf * ((g - sg_n) - xh * sgx_n);
      }
    }
  }
}

}  // namespace mtlssl

using namespace mtlssl;

extern "C" {

int mtlssl_batch_norm_train_fwd(const float* x, const float* gamma, const float* beta, float* y, float* save_mean,
                                float* save_inv_std, float* moving_mean, float* moving_var, int64_t rows, int C,
                                float eps, float f, int epilogue, mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(x && y && save_mean && save_inv_std, "batch_norm_train_fwd: null x / y / save_mean / save_inv_std");
  MTLSSL_REQUIRE(rows >= 1 && rows <= (1ll << 24) && C >= 1, "batch_norm_train_fwd: rows must be in [1, 2^24] and C >= 1");
  MTLSSL_REQUIRE((moving_mean == nullptr) == (moving_var == nullptr),
                 "batch_norm_train_fwd: moving_mean and moving_var go together");
  MTLSSL_REQUIRE((epilogue & ~(MTLSSL_EPI_RELU | MTLSSL_EPI_RELU6)) == 0 &&
                     epilogue != (MTLSSL_EPI_RELU | MTLSSL_EPI_RELU6),
                 "batch_norm_train_fwd: epilogue is 0, RELU or RELU6");
  hipLaunchKernelGGL(k_batch_norm_train_fwd, dim3(cdiv(C, BN_CH)), dim3(BN_THREADS), 0, S(stream), x, gamma, beta, y,
                     save_mean, save_inv_std, moving_mean, moving_var, rows, C, eps, f, epilogue);
  return check_launch("batch_norm_train_fwd");
}

int mtlssl_batch_norm_train_bwd(const float* x, const float* dy, const float* y, const float* gamma,
                                const float* save_mean, const float* save_inv_std, float* dx, float* dgamma,
                                float* dbeta, int64_t rows, int C, float accum, int mask_epilogue,
                                mtlssl_stream_t stream) {
  MTLSSL_REQUIRE(x && dy && dx && save_mean && save_inv_std, "batch_norm_train_bwd: null x / dy / dx / saved statistics");
  MTLSSL_REQUIRE(rows >= 1 && rows <= (1ll << 24) && C >= 1, "batch_norm_train_bwd: rows must be in [1, 2^24] and C >= 1");
  MTLSSL_REQUIRE(mask_epilogue == 0 || mask_epilogue == MTLSSL_EPI_MASK || mask_epilogue == MTLSSL_EPI_MASK6,
                 "batch_norm_train_bwd: mask_epilogue is 0, MASK or MASK6");
  MTLSSL_REQUIRE(mask_epilogue == 0 || y != nullptr, "batch_norm_train_bwd: a mask needs y");
  hipLaunchKernelGGL(k_batch_norm_train_bwd, dim3(cdiv(C, BN_CH)), dim3(BN_THREADS), 0, S(stream), x, dy, y, gamma,
                     save_mean, save_inv_std, dx, dgamma, dbeta, rows, C, accum, mask_epilogue);
  return check_launch("batch_norm_train_bwd");
}

}  // extern "C"
