// The convolution epilogue (the MTLSSL_EPI_* flags of include/mtlssl_hip.h), stated once for every kernel that ends a
// convolution — the tile engines, the split-K folds, the scalar and small-GEMM kernels, the Winograd output transform,
// the parity scatter — and for the depthwise and batch-norm kernels that share its activations:
//
//   forward        : v + bias, + residual, then ReLU | ReLU6 | tanh                          epilogue_fwd
//   input gradient : v + residual, + previous contents (ACCUM), then the ReLU | ReLU6 mask   epilogue_dgrad
//
// Only the arithmetic and its order live here. The operands stay with the call site, which knows their vector width, row
// strides and prefetch: each one is passed as EPI_OPERAND(expression) and evaluated only under its flag, so a pointer
// that the flags do not ask for is never read. V is float or floatx4. FLAGS names the flags a site can be launched with
// (what its host entry admits): the code of the others is not instantiated.
#pragma once
#include "common.h"

namespace mtlssl {

typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int ACT_ANY = MTLSSL_EPI_RELU | MTLSSL_EPI_RELU6 | MTLSSL_EPI_TANH;
constexpr int MASK_ANY = MTLSSL_EPI_MASK | MTLSSL_EPI_MASK6;
constexpr int FWD_ANY = MTLSSL_EPI_BIAS | MTLSSL_EPI_RESIDUAL | ACT_ANY;

// inlined as early as the chains themselves, so that a call site compiles as if it spelled the chain out
#define EPI_OPERAND(expr) [&]() __attribute__((always_inline)) { return (expr); }

template <int FLAGS>
__device__ __forceinline__ bool epi_has(int epi, int flag) { return (FLAGS & flag) && (epi & flag); }

// The activation applied to X in place. X is a float or ONE LANE of a floatx4 (a lane cannot be bound to a reference, hence
// a macro): the vector form updates lane by lane, which is the form the tile engine's schedule was tuned and measured with.
#define EPI_ACT_IN_PLACE(X)                                                  \
  do {                                                                       \
    if (epi_has<FLAGS>(epi, MTLSSL_EPI_RELU)) X = fmaxf(X, 0.f);             \
    if (epi_has<FLAGS>(epi, MTLSSL_EPI_RELU6)) X = fminf(fmaxf(X, 0.f), 6.f); \
    if (epi_has<FLAGS>(epi, MTLSSL_EPI_TANH)) X = tanhf(X);                  \
  } while (0)
template <int FLAGS = ACT_ANY>
__device__ __forceinline__ float act_fwd(float v, int epi) {
  EPI_ACT_IN_PLACE(v);
  return v;
}
template <int FLAGS = ACT_ANY>
__device__ __forceinline__ floatx4 act_fwd(floatx4 v, int epi) {
#pragma unroll
  for (int q = 0; q < 4; ++q) EPI_ACT_IN_PLACE(v[q]);
  return v;
}
#undef EPI_ACT_IN_PLACE
// ReLU / ReLU6 backward: pass the gradient where the activation was in its linear range.
__device__ __forceinline__ float act_mask(float g, float y, int epi) {
  bool on = y > 0.f && (!(epi & MTLSSL_EPI_MASK6) || y < 6.f);
  return on ? g : 0.f;
}
__device__ __forceinline__ floatx4 act_mask(floatx4 g, floatx4 y, int epi) {
#pragma unroll
  for (int q = 0; q < 4; ++q) g[q] = act_mask(g[q], y[q], epi);
  return g;
}

template <int FLAGS = FWD_ANY, typename V, typename Bias, typename Res>
__device__ __forceinline__ V epilogue_fwd(V v, int epi, Bias bias, Res residual) {
  if (epi_has<FLAGS>(epi, MTLSSL_EPI_BIAS)) v += bias();
  if (epi_has<FLAGS>(epi, MTLSSL_EPI_RESIDUAL)) v += residual();
  return act_fwd<FLAGS>(v, epi);
}
template <typename V, typename Res, typename Prev, typename Mask>
__device__ __forceinline__ V epilogue_dgrad(V v, int epi, Res residual, Prev previous, Mask mask_ref) {
  if (epi & MTLSSL_EPI_RESIDUAL) v += residual();
  if (epi & MTLSSL_EPI_ACCUM) v += previous();
  if (epi & MASK_ANY) v = act_mask(v, mask_ref(), epi);
  return v;
}

}  // namespace mtlssl
