// What the step kernels of steps.hip and nullspace.hip share: the 4-elements-per-thread launch, the 16-byte accesses with their scalar fall-back, the
// noise of a draw, and the data prediction x0_pre of a prediction kind.  An includer sets `#pragma clang fp contract(off)` in front of this header:
// every expression below is written operation by operation.
#pragma once
#include "ops.h"
#include "philox.h"

namespace {

// Every kernel launched through launch_ew4 handles 4 consecutive elements per thread (16-B accesses) with a scalar tail.
template <typename F>
__global__ void __launch_bounds__(256) ew4_kernel(int64_t n, F f) {
  const int64_t i4 = ((int64_t)blockIdx.x * 256 + threadIdx.x);
  const int64_t i = i4 * 4;
  if (i >= n) return;
  f(i, i4, (int)((n - i) < 4 ? (n - i) : 4));
}

template <typename F>
int launch_ew4(int64_t n, hipStream_t s, F f) {
  if (n <= 0) return 0;
  const int64_t nthreads = (n + 3) / 4;
  hipLaunchKernelGGL(ew4_kernel<F>, dim3((unsigned)((nthreads + 255) / 256)), dim3(256), 0, s, n, f);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

__device__ inline void ld4(const float* p, int64_t i, int cnt, float (&v)[4]) {
  if (cnt == 4 && ((reinterpret_cast<uintptr_t>(p + i) & 15) == 0)) {
    f32x4 t = *reinterpret_cast<const f32x4*>(p + i);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    for (int j = 0; j < 4; ++j) v[j] = j < cnt ? p[i + j] : 0.f;
  }
}
__device__ inline void st4(float* p, int64_t i, int cnt, const float (&v)[4]) {
  if (cnt == 4 && ((reinterpret_cast<uintptr_t>(p + i) & 15) == 0)) {
    *reinterpret_cast<f32x4*>(p + i) = f32x4{v[0], v[1], v[2], v[3]};
  } else {
    for (int j = 0; j < cnt; ++j) p[i + j] = v[j];
  }
}
__device__ inline void noise4(const float* z, int use_philox, uint64_t seed, uint64_t offset4, int64_t i, int64_t i4, int cnt,
                              float (&zz)[4]) {
  if (z) ld4(z, i, cnt, zz);
  else if (use_philox) randn4(seed, offset4 + (uint64_t)i4, zz);
  else { zz[0] = zz[1] = zz[2] = zz[3] = 0.f; }
}

// x0_hat before its clip, the ONE expression every predictor step and x0_shape_stats_kernel evaluate (product, product, difference: the includers have
// contraction off), so that the order statistic the stats kernel selects is an element of what the step clamps
__device__ inline float x0_pre(float c_recip, float c_recipm1, float x, float e) { return c_recip * x - c_recipm1 * e; }
// What the network output `o` stands for (PRED_*, ops.h), resolved at compile time: x0_pre of the kind.  eps: the expression above on the step's own
// c_recip, c_recipm1 (nothing carried).  x0: the output itself, no arithmetic, x is not read for it.  v (Salimans & Ho 2022): sa x - sb o with sa =
// sqrt_alphas_cumprod, sb = sqrt_one_minus_alphas_cumprod of the step, the same three roundings.
template <int K> struct Pred;
template <> struct Pred<PRED_EPS> {
  __device__ inline float pre(float c_recip, float c_recipm1, float x, float o) const { return x0_pre(c_recip, c_recipm1, x, o); }
};
template <> struct Pred<PRED_X0> {
  __device__ inline float pre(float, float, float, float o) const { return o; }
};
template <> struct Pred<PRED_V> {
  float sa, sb;
  __device__ inline float pre(float, float, float x, float o) const { return x0_pre(sa, sb, x, o); }
};
// Four elements of a per-image strided tensor: element r of image b sits at p[b * stride + r] (the eps channels of a [B, 2C, H, W] network output:
// per = C H W, stride = 2 per).  i indexes the dense [B][per] state; a group of four may straddle images when per % 4 != 0.
__device__ inline void ld4_strided(const float* p, int64_t per, int64_t stride, int64_t i, int cnt, float (&v)[4]) {
  int64_t img = i / per, r = i - img * per;
  if (cnt == 4 && r + 4 <= per) { ld4(p + img * stride + r, 0, 4, v); return; }
#pragma unroll
  for (int l = 0; l < 4; ++l) v[l] = 0.f;
  for (int l = 0; l < cnt; ++l) {
    while (r >= per) { r -= per; ++img; }
    v[l] = p[img * stride + r];
    ++r;
  }
}
// eps of image b at eps + b * stride; stride == per: the contiguous read.  The same rule reads v (the variance channels) at eps + per.
__device__ inline void ld4_eps(const float* eps, int64_t per, int64_t stride, int64_t i, int cnt, float (&v)[4]) {
  if (stride == per) ld4(eps, i, cnt, v);
  else ld4_strided(eps, per, stride, i, cnt, v);
}
// run f(Pred<K>) for a prediction kind (checked by the caller)
template <typename F> int pred_form(int pred, float sa, float sb, F&& f) {
  if (pred == PRED_X0) return f(Pred<PRED_X0>{});
  if (pred == PRED_V) return f(Pred<PRED_V>{sa, sb});
  return f(Pred<PRED_EPS>{});
}
// The host side of the DDIM(eta) step's two coefficients: sqrt(acp_prev) and sqrt(max(1 - acp_prev - sigma^2, 0)), 1 - acp_prev - sigma^2 left to
// right, sigma^2 rounded
struct DdimEta { float sa, sb; };
inline DdimEta ddim_eta_coefs(float acp_prev, float sigma) {
  const float s2 = sigma * sigma;
  const float r = 1.0f - acp_prev;
  return {sqrtf(acp_prev), sqrtf(fmaxf(r - s2, 0.f))};
}

}  // namespace
