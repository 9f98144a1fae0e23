// Fused elementwise / reduction kernels of the adaptive Dormand-Prince 5(4) integrator (the reference's default FID
// solver: torchdiffeq.odeint(..., method="dopri5"), cifar10/compute_fid.py:80-85, mnist/utils_mnist.py:101-108).
// The step-size controller itself runs on the host (it needs one scalar per step anyway); these kernels replace the
// dozens of eager elementwise launches torchdiffeq issues per step: stage combination, error norm, dense output.
#include "ops.h"

namespace {

struct KPtrs { const float* k[7]; float c[7]; };

__global__ void __launch_bounds__(256) rk_combine_kernel(float* out, const float* y0, KPtrs kp, int nk, int64_t n, int vec) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n && vec) {   // vec: every pointer is 16-byte aligned (checked once by the launcher); a view at an odd storage offset goes scalar
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nk; ++j) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kp.k[j] + i);
      const float c = kp.c[j];
      acc = f32x4{acc[0] + kv[0] * c, acc[1] + kv[1] * c, acc[2] + kv[2] * c, acc[3] + kv[3] * c};
    }
    f32x4 y = y0 ? *reinterpret_cast<const f32x4*>(y0 + i) : f32x4{0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>(out + i) = f32x4{y[0] + acc[0], y[1] + acc[1], y[2] + acc[2], y[3] + acc[3]};
  } else {
    const int64_t end = i + 4 < n ? i + 4 : n;
    for (int64_t e = i; e < end; ++e) {
      float acc = 0.f;
      for (int j = 0; j < nk; ++j) acc += kp.k[j][e] * kp.c[j];
      out[e] = (y0 ? y0[e] : 0.f) + acc;
    }
  }
}

struct StagePtrs { const float* k[4]; float c[4]; };

// (x * 127.5 + 128).clip(0, 255).to(uint8) of quantize_u8_launch (steps.hip, compiled with contraction off): product and sum rounded separately
__device__ __forceinline__ uint8_t stage_u8(float x) {
#pragma clang fp contract(off)
  const float p = x * 127.5f;
  const float v = clip_nan(p + 128.f, 0.f, 255.f);
  return (uint8_t)(int)v;
}

// One stage of a fixed-step explicit Runge-Kutta sampler: out = y0 + sum_j c_j k_j, summed as rk_combine_kernel does, with the step's other outputs
// in the same launch: copy_out (the trajectory slot) and u8_out (the image bytes of the rounded fp32 result).  out may be y0 (the state updated in
// place: every thread reads its own elements before it writes them).
__global__ void __launch_bounds__(256) rk_stage_kernel(float* out, const float* y0, StagePtrs kp, int nk, int64_t n, float* copy_out,
                                                     uint8_t* u8_out, int vec) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  if (i + 4 <= n && vec) {   // vec: every fp32 pointer is 16-byte aligned and u8_out 4-byte aligned (checked once by the launcher)
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nk; ++j) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kp.k[j] + i);
      const float c = kp.c[j];
      acc = f32x4{acc[0] + kv[0] * c, acc[1] + kv[1] * c, acc[2] + kv[2] * c, acc[3] + kv[3] * c};
    }
    const f32x4 y = *reinterpret_cast<const f32x4*>(y0 + i);
    const f32x4 r = f32x4{y[0] + acc[0], y[1] + acc[1], y[2] + acc[2], y[3] + acc[3]};
    *reinterpret_cast<f32x4*>(out + i) = r;
    if (copy_out) *reinterpret_cast<f32x4*>(copy_out + i) = r;
    if (u8_out)
      *reinterpret_cast<uint32_t*>(u8_out + i) = (uint32_t)stage_u8(r[0]) | ((uint32_t)stage_u8(r[1]) << 8) | ((uint32_t)stage_u8(r[2]) << 16) |
                                                 ((uint32_t)stage_u8(r[3]) << 24);
  } else {
    const int64_t end = i + 4 < n ? i + 4 : n;
    for (int64_t e = i; e < end; ++e) {
      float acc = 0.f;
      for (int j = 0; j < nk; ++j) acc += kp.k[j][e] * kp.c[j];
      const float r = y0[e] + acc;
      out[e] = r;
      if (copy_out) copy_out[e] = r;
      if (u8_out) u8_out[e] = stage_u8(r);
    }
  }
}

// g = ku + w * (kc - ku): the difference, the product and the sum each rounded to fp32, in that order
__device__ __forceinline__ float cfg_mix(float kc, float ku, float w) {
#pragma clang fp contract(off)
  const float d = kc - ku;
  const float p = w * d;
  return ku + p;
}

// rk_stage_kernel over classifier-free-guided derivatives: k_j holds 2n values, the conditional evaluation in [0, n) and the unconditional one in
// [n, 2n) (one network call at twice the batch); g_j = cfg_mix of the two and out = y0 + sum_j c_j g_j, summed as rk_stage_kernel does.  w_dev
// (optional): one scale per image of `per` elements instead of the scalar w.  y0 may be null (no base term: with nk = 1, c = 1 the guided field
// itself).  dup: the result also goes to out[n + e], the second half of a duplicated state.  out may be y0: a thread reads its own elements first.
__global__ void __launch_bounds__(256) cfg_stage_kernel(float* out, const float* y0, StagePtrs kp, int nk, int64_t n, float w, const float* w_dev,
                                                      int64_t per, int dup, float* copy_out, uint8_t* u8_out, int vec) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const int cnt = (int)(n - i < 4 ? n - i : 4);
  float wv[4] = {w, w, w, w};
  if (w_dev) {   // a group of four may straddle images when per % 4 != 0
    int64_t img = i / per, r = i - img * per;
    for (int l = 0; l < cnt; ++l) {
      while (r >= per) { r -= per; ++img; }
      wv[l] = w_dev[img];
      ++r;
    }
  }
  if (cnt == 4 && vec) {   // vec: every fp32 pointer and every half base p + n is 16-byte aligned, u8_out 4-byte aligned (checked once by the launcher)
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < nk; ++j) {
      const f32x4 kc = *reinterpret_cast<const f32x4*>(kp.k[j] + i);
      const f32x4 ku = *reinterpret_cast<const f32x4*>(kp.k[j] + n + i);
      const f32x4 g = f32x4{cfg_mix(kc[0], ku[0], wv[0]), cfg_mix(kc[1], ku[1], wv[1]), cfg_mix(kc[2], ku[2], wv[2]), cfg_mix(kc[3], ku[3], wv[3])};
      const float c = kp.c[j];
      acc = f32x4{acc[0] + g[0] * c, acc[1] + g[1] * c, acc[2] + g[2] * c, acc[3] + g[3] * c};
    }
    f32x4 r = acc;
    if (y0) { const f32x4 y = *reinterpret_cast<const f32x4*>(y0 + i); r = f32x4{y[0] + acc[0], y[1] + acc[1], y[2] + acc[2], y[3] + acc[3]}; }
    *reinterpret_cast<f32x4*>(out + i) = r;
    if (dup) *reinterpret_cast<f32x4*>(out + n + i) = r;
    if (copy_out) *reinterpret_cast<f32x4*>(copy_out + i) = r;
    if (u8_out)
      *reinterpret_cast<uint32_t*>(u8_out + i) = (uint32_t)stage_u8(r[0]) | ((uint32_t)stage_u8(r[1]) << 8) | ((uint32_t)stage_u8(r[2]) << 16) |
                                                 ((uint32_t)stage_u8(r[3]) << 24);
  } else {
    for (int l = 0; l < cnt; ++l) {
      const int64_t e = i + l;
      float acc = 0.f;
      for (int j = 0; j < nk; ++j) acc += cfg_mix(kp.k[j][e], kp.k[j][e + n], wv[l]) * kp.c[j];
      const float r = y0 ? y0[e] + acc : acc;
      out[e] = r;
      if (dup) out[e + n] = r;
      if (copy_out) copy_out[e] = r;
      if (u8_out) u8_out[e] = stage_u8(r);
    }
  }
}

// sum_i ((a_i - sub_i) / (atol + rtol * max(|b_i|, |b2_i|)))^2  accumulated into *out (fp64 atomics, one per block)
__global__ void __launch_bounds__(256) rk_sqnorm_kernel(const float* a, const float* sub, const float* b, const float* b2, float atol,
                                                      float rtol, int64_t n, double* out) {
  __shared__ double sh[4];
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float num = a[i] - (sub ? sub[i] : 0.f);
    float mag = b ? fabsf(b[i]) : 0.f;
    if (b2) mag = fmaxf(mag, fabsf(b2[i]));
    const float r = num / (atol + rtol * mag);
    acc += (double)r * (double)r;
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out, sh[0] + sh[1] + sh[2] + sh[3]);
}

// torchdiffeq dense output (interp.py _interp_fit / _interp_evaluate): quartic through y0, y_mid, y1 with end slopes f0, f1
__global__ void __launch_bounds__(256) rk_interp_kernel(float* out, const float* y0, const float* y1, const float* ym, const float* f0,
                                                      const float* f1, float dt, float x, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float a = 2.f * dt * (f1[i] - f0[i]) - 8.f * (y1[i] + y0[i]) + 16.f * ym[i];
  const float b = dt * (5.f * f0[i] - 3.f * f1[i]) + 18.f * y0[i] + 14.f * y1[i] - 32.f * ym[i];
  const float c = dt * (f1[i] - 4.f * f0[i]) - 11.f * y0[i] - 5.f * y1[i] + 16.f * ym[i];
  const float d = dt * f0[i], e = y0[i];
  out[i] = (((a * x + b) * x + c) * x + d) * x + e;
}

}  // namespace

int rk_combine_launch(float* out, const float* y0, const float* const* k, const float* c, int nk, int64_t n, hipStream_t s) {
  MI355_REQUIRE(nk >= 0 && nk <= 7, -1, "rk_combine: bad argument");
  if (n <= 0) return 0;   // an empty tensor (its pointer may be null): nothing to do, and a zero-sized grid is a launch error
  MI355_REQUIRE(out, -1, "rk_combine: bad argument");
  KPtrs kp;
  uintptr_t bits = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(y0);   // a null y0 adds no bits
  for (int j = 0; j < 7; ++j) {
    kp.k[j] = j < nk ? k[j] : nullptr; kp.c[j] = j < nk ? c[j] : 0.f;
    MI355_REQUIRE(j >= nk || k[j], -1, "rk_combine: null stage pointer");
    bits |= reinterpret_cast<uintptr_t>(kp.k[j]);
  }
  const int64_t nth = (n + 3) / 4;
  hipLaunchKernelGGL(rk_combine_kernel, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, s, out, y0, kp, nk, n, (int)((bits & 15) == 0));
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int rk_stage_launch(float* out, const float* y0, const float* const* k, const float* c, int nk, int64_t n, float* copy_out, uint8_t* u8_out,
                    hipStream_t s) {
  MI355_REQUIRE(nk >= 1 && nk <= 4, -1, "rk_stage: 1 to 4 stage derivatives");
  if (n <= 0) return 0;   // an empty tensor (its pointers may be null): nothing to do
  MI355_REQUIRE(out && y0 && k && c, -1, "rk_stage: null argument");
  StagePtrs kp;
  uintptr_t bits = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(y0) | reinterpret_cast<uintptr_t>(copy_out);   // null adds no bits
  for (int j = 0; j < 4; ++j) {
    MI355_REQUIRE(j >= nk || k[j], -1, "rk_stage: null stage pointer");
    kp.k[j] = j < nk ? k[j] : nullptr; kp.c[j] = j < nk ? c[j] : 0.f;
    bits |= reinterpret_cast<uintptr_t>(kp.k[j]);
  }
  const int vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(u8_out) & 3) == 0;
  const int64_t nth = (n + 3) / 4;
  hipLaunchKernelGGL(rk_stage_kernel, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, s, out, y0, kp, nk, n, copy_out, u8_out, vec);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int cfg_stage_launch(float* out, const float* y0, const float* const* k, const float* c, int nk, int64_t n, float w, const float* w_dev, int64_t per,
                     int dup, float* copy_out, uint8_t* u8_out, hipStream_t s) {
  MI355_REQUIRE(nk >= 1 && nk <= 4, -1, "cfg_stage: 1 to 4 stage derivatives");
  if (n <= 0) return 0;   // an empty tensor (its pointers may be null): nothing to do
  MI355_REQUIRE(out && k && c, -1, "cfg_stage: null argument");
  MI355_REQUIRE(!w_dev || (per > 0 && n % per == 0), -1, "cfg_stage: per-image scales need n to be whole images of elems_per_image elements");
  StagePtrs kp;
  uintptr_t bits = reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(y0) | reinterpret_cast<uintptr_t>(copy_out);   // null adds no bits
  for (int j = 0; j < 4; ++j) {
    MI355_REQUIRE(j >= nk || k[j], -1, "cfg_stage: null stage pointer");
    kp.k[j] = j < nk ? k[j] : nullptr; kp.c[j] = j < nk ? c[j] : 0.f;
    bits |= reinterpret_cast<uintptr_t>(kp.k[j]);
  }
  bits |= (uintptr_t)((n & 3) * 4);   // the second halves start n floats behind aligned bases
  const int vec = (bits & 15) == 0 && (reinterpret_cast<uintptr_t>(u8_out) & 3) == 0;
  const int64_t nth = (n + 3) / 4;
  hipLaunchKernelGGL(cfg_stage_kernel, dim3((unsigned)((nth + 255) / 256)), dim3(256), 0, s, out, y0, kp, nk, n, w, w_dev, per > 0 ? per : 1, dup, copy_out,
                     u8_out, vec);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int rk_sqnorm_launch(const float* a, const float* sub, const float* b, const float* b2, float atol, float rtol, int64_t n, double* out,
                     hipStream_t s) {
  if (n <= 0) return 0;   // the sum over no elements adds nothing
  MI355_REQUIRE(a && out, -1, "rk_sqnorm: null argument");
  int64_t blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(rk_sqnorm_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a, sub, b, b2, atol, rtol, n, out);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int rk_interp_launch(float* out, const float* y0, const float* y1, const float* ym, const float* f0, const float* f1, float dt, float x,
                     int64_t n, hipStream_t s) {
  if (n <= 0) return 0;
  MI355_REQUIRE(out && y0 && y1 && ym && f0 && f1, -1, "rk_interp: null argument");
  hipLaunchKernelGGL(rk_interp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, out, y0, y1, ym, f0, f1, dt, x, n);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
