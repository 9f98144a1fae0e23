// The variational bound (bits/dim) of a DDPM net, step by step: the per-image KL of step k > 0, the discretised Gaussian decoder of step 0, the
// two diagnostics of guided-diffusion's calc_bpd_loop (the squared error of the data prediction and of eps), and the prior term with the total.
//
// No reference counterpart: the reference trains with the simple loss alone (AD/image_diffusion/loss_functions.py) and never evaluates the bound.
// The formulas are Ho et al. 2020 (eq. 5, the decoder of section 3.3) and Nichol & Dhariwal 2021 (eq. 15), stated in include/mi355_sampler.h at
// mi355_ddpm_vlb and restated in fp64 by tests/vlb_ref.py.
//
// Streaming kernels of a few hundred KB per launch, one 256-thread workgroup per image as image_metrics_kernel is laid out.  Every per-element
// operation is fp64 on the fp32 values widened; the sums are fp64 in a fixed order (per-thread strided sum, wave butterfly, four-entry LDS combine,
// no atomics), so two runs give the same bits; each output number is rounded to fp32 once.
#include <cmath>

#include "ops.h"

// the fp64 expressions are evaluated operation by operation as they are written (and as the restatement evaluates them)
#pragma clang fp contract(off)

#include "philox.h"

namespace {

constexpr double LN2 = 0.6931471805599453;

struct VlbScalars { double c_recip, c_recipm1, coef1, coef2, lq, lp_fixed, min_log, max_log, sa, sb; int pred; };

// four consecutive floats: one 16-byte load where the address allows it
__device__ inline void ld4v(const float* p, float (&v)[4]) {
  if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else {
    v[0] = p[0]; v[1] = p[1]; v[2] = p[2]; v[3] = p[3];
  }
}
// Elements g .. g + 3 of the draw at Philox counter base off4, g the index in the dense [batch][per] state: they straddle two counters unless
// g % 4 == 0.  sh = g & 3 is the same for every group of an image, so the switch is uniform.
__device__ inline void philox4_at(uint64_t seed, uint64_t off4, int64_t g, float (&zz)[4]) {
  float a[4], b[4];
  const uint64_t c = off4 + (uint64_t)(g >> 2);
  randn4(seed, c, a);
  const int sh = (int)(g & 3);
  if (sh == 0) { zz[0] = a[0]; zz[1] = a[1]; zz[2] = a[2]; zz[3] = a[3]; return; }
  randn4(seed, c + 1, b);
  switch (sh) {
    case 1: zz[0] = a[1]; zz[1] = a[2]; zz[2] = a[3]; zz[3] = b[0]; break;
    case 2: zz[0] = a[2]; zz[1] = a[3]; zz[2] = b[0]; zz[3] = b[1]; break;
    default: zz[0] = a[3]; zz[1] = b[0]; zz[2] = b[1]; zz[3] = b[2]; break;
  }
}
__device__ inline float philox1_at(uint64_t seed, uint64_t off4, int64_t g) {
  float a[4];
  randn4(seed, off4 + (uint64_t)(g >> 2), a);
  switch ((int)(g & 3)) {
    case 0: return a[0];
    case 1: return a[1];
    case 2: return a[2];
    default: return a[3];
  }
}

// the three fp64 sums of a workgroup, in a fixed order; every thread returns with the totals
template <int N>
__device__ inline void block_sum(double (&v)[N], double (*sh)[4]) {
#pragma unroll
  for (int j = 0; j < N; ++j)
    for (int o = 32; o > 0; o >>= 1) v[j] += __shfl_xor(v[j], o);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int j = 0; j < N; ++j) sh[j][threadIdx.x >> 6] = v[j];
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < N; ++j) v[j] = (sh[j][0] + sh[j][1]) + (sh[j][2] + sh[j][3]);
}

// Phi, the standard normal CDF.  Exact: through erfc, whose far tail keeps its relative accuracy.  Tanh: guided-diffusion's approximation.
__device__ inline double phi_erfc(double a) { return 0.5 * erfc(-a / 1.4142135623730951); }
__device__ inline double phi_tanh(double a) { return 0.5 * (1.0 + tanh(0.7978845608028654 * (a + 0.044715 * (a * a * a)))); }

// -log p(x0 | x_1) of one element under the 8-bit discretised Gaussian N(mean_p, exp(lp)).  CDF 0: every probability is taken where the values
// are at most 0.5 (the upper open bin as Phi(-a-), an inner bin right of the mean as Phi(-a-) - Phi(-a+)); CDF 1: the three expressions verbatim.
template <int CDF>
__device__ inline double decoder_nll(double x0, double mean_p, double lp) {
  const double c = x0 - mean_p;
  const double s = exp(-0.5 * lp);
  const double ap = s * (c + 1.0 / 255.0), am = s * (c - 1.0 / 255.0);
  double p;
  if (CDF == 0) {
    if (x0 < -0.999) p = phi_erfc(ap);
    else if (x0 > 0.999) p = phi_erfc(-am);
    else p = c > 0.0 ? phi_erfc(-am) - phi_erfc(-ap) : phi_erfc(ap) - phi_erfc(am);
  } else {
    if (x0 < -0.999) p = phi_tanh(ap);
    else if (x0 > 0.999) p = 1.0 - phi_tanh(am);
    else p = phi_tanh(ap) - phi_tanh(am);
  }
  return -log(p < 1e-12 ? 1e-12 : p);   // a NaN stays one
}

// one element into the three running sums acc = { vb term, (x0_hat - x0)^2, (out - target)^2 }, target what a net of the kind is trained on: z for
// eps, x0 for x0, sa z - sb x0 for v; x0_hat from x0_pre of the kind (c.pred is uniform over the launch)
template <bool K0, int CDF>
__device__ inline void vlb_elem(const VlbScalars& c, bool learned, bool clip, float x0f, float xkf, float ef, float vf, float zf, double (&acc)[3]) {
  const double x0 = (double)x0f, xk = (double)xkf, eps = (double)ef, z = (double)zf;
  double xh = c.pred == PRED_X0 ? eps : (c.pred == PRED_V ? c.sa * xk - c.sb * eps : c.c_recip * xk - c.c_recipm1 * eps);
  if (clip) xh = xh < -1.0 ? -1.0 : (xh > 1.0 ? 1.0 : xh);
  const double mean_p = c.coef1 * xh + c.coef2 * xk;
  double lp = c.lp_fixed;
  if (learned) {
    const double frac = ((double)vf + 1.0) / 2.0;
    lp = frac * c.max_log + (1.0 - frac) * c.min_log;
  }
  if (K0) {
    acc[0] += decoder_nll<CDF>(x0, mean_p, lp);
  } else {
    const double mean_q = c.coef1 * x0 + c.coef2 * xk;
    const double d = mean_q - mean_p;
    acc[0] += 0.5 * (-1.0 + lp - c.lq + exp(c.lq - lp) + d * d * exp(-lp));
  }
  const double target = c.pred == PRED_X0 ? x0 : (c.pred == PRED_V ? c.sa * z - c.sb * x0 : z);
  const double dx = xh - x0, de = eps - target;
  acc[1] += dx * dx;
  acc[2] += de * de;
}

// Image b = blockIdx.x.  The groups of four are anchored where x0 of the image becomes 16-byte aligned: a scalar head of up to three elements, the
// body in 16-byte loads for every operand that shares x0's alignment (the others fall back to four 4-byte loads, still coalesced), a scalar tail.
template <bool K0, int CDF>
__global__ void __launch_bounds__(256) vlb_terms_kernel(const float* x0, const float* xk, const float* out, int64_t out_stride, const float* z,
                                                        int use_philox, uint64_t seed, uint64_t off4, VlbScalars c, int learned, int clip, float* dst,
                                                        int64_t dst_stride, int64_t per) {
  __shared__ double sh[3][4];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x, base = b * per;
  const float* px0 = x0 + base;
  const float* pxk = xk + base;
  const float* pe = out + b * out_stride;
  const float* pv = pe + per;   // dereferenced iff learned
  const float* pz = z ? z + base : nullptr;
  const bool lv = learned != 0, cl = clip != 0;
  double acc[3] = {0.0, 0.0, 0.0};
  auto one = [&](int64_t r) {
    const float zf = pz ? pz[r] : philox1_at(seed, off4, base + r);
    vlb_elem<K0, CDF>(c, lv, cl, px0[r], pxk[r], pe[r], lv ? pv[r] : 0.f, zf, acc);
  };
  int64_t head = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(px0) >> 2) & 3)) & 3);
  if (head > per) head = per;
  const int64_t groups = (per - head) / 4, tail = head + groups * 4;
  if (tid < head) one(tid);
  for (int64_t g = tid; g < groups; g += 256) {
    const int64_t r = head + g * 4;
    float a0[4], ak[4], ae[4], av[4] = {0.f, 0.f, 0.f, 0.f}, az[4];
    ld4v(px0 + r, a0); ld4v(pxk + r, ak); ld4v(pe + r, ae);
    if (lv) ld4v(pv + r, av);
    if (pz) ld4v(pz + r, az);
    else philox4_at(seed, off4, base + r, az);
#pragma unroll
    for (int j = 0; j < 4; ++j) vlb_elem<K0, CDF>(c, lv, cl, a0[j], ak[j], ae[j], av[j], az[j], acc);
  }
  if (tail + tid < per) one(tail + tid);
  block_sum(acc, sh);
  if (tid == 0) {
    float* o = dst + b * dst_stride;
    const double n = (double)per;
    o[0] = (float)(acc[0] / n / LN2);
    o[1] = (float)(acc[1] / n);
    o[2] = (float)(acc[2] / n);
  }
}

// KL(q(x_K | x_0) || N(0, 1)) per image in bits/dim, and the total of the image's K step terms with it
__global__ void __launch_bounds__(256) vlb_prior_kernel(const float* x0, double sa, double L, double eL, const float* terms, int64_t terms_stride, int K,
                                                        float* summary, int64_t per) {
  __shared__ double sh[2][4];
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const float* p = x0 + b * per;
  double acc[2] = {0.0, 0.0};
  auto one = [&](float xf) {
    const double m = sa * (double)xf;
    acc[0] += 0.5 * (-1.0 - L + eL + m * m);
  };
  int64_t head = (int64_t)((4 - ((reinterpret_cast<uintptr_t>(p) >> 2) & 3)) & 3);
  if (head > per) head = per;
  const int64_t groups = (per - head) / 4, tail = head + groups * 4;
  if (tid < head) one(p[tid]);
  for (int64_t g = tid; g < groups; g += 256) {
    float a[4];
    ld4v(p + head + g * 4, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) one(a[j]);
  }
  if (tail + tid < per) one(p[tail + tid]);
  if (terms)
    for (int k = tid; k < K; k += 256) acc[1] += (double)terms[b * terms_stride + 3 * (int64_t)k];
  block_sum(acc, sh);
  if (tid == 0) {
    const float prior = (float)(acc[0] / (double)per / LN2);
    summary[b * 2] = prior;
    if (terms) summary[b * 2 + 1] = (float)(acc[1] + (double)prior);
  }
}

}  // namespace

int vlb_terms_launch(const float* x0, const float* xk, const float* out, int64_t out_stride, const float* z, int use_philox, uint64_t seed,
                     uint64_t offset, const VlbStep& st, float* dst, int64_t dst_stride, int batch, int64_t per, hipStream_t s) {
  MI355_REQUIRE(st.k_is_zero == 0 || st.k_is_zero == 1, -1, "vlb_terms: k_is_zero must be 0 or 1");
  MI355_REQUIRE(st.learned == 0 || st.learned == 1, -1, "vlb_terms: learned must be 0 (model_log) or 1 (the range min_log, max_log)");
  MI355_REQUIRE(st.cdf == 0 || st.cdf == 1, -1, "vlb_terms: cdf must be 0 (exact, erfc) or 1 (the tanh approximation)");
  MI355_REQUIRE(st.clip == 0 || st.clip == 1, -1, "vlb_terms: clip_denoised must be 0 or 1");
  MI355_REQUIRE(st.pred >= PRED_EPS && st.pred <= PRED_V, -1, "vlb_terms: the prediction kind must be 0 (eps), 1 (x0) or 2 (v)");
  if (st.pred == PRED_V) MI355_REQUIRE(std::isfinite(st.sa) && std::isfinite(st.sb), -1, "vlb_terms: sa and sb must be finite");
  MI355_REQUIRE(per > 0, -1, "vlb_terms: elems_per_image must be > 0");
  MI355_REQUIRE(batch >= 0, -1, "vlb_terms: batch must be >= 0");
  MI355_REQUIRE(out_stride >= (st.learned ? 2 : 1) * per, -1,
                "vlb_terms: out_stride must be >= elems_per_image (learned: >= 2 * elems_per_image, the variance channels sit behind eps)");
  MI355_REQUIRE(dst_stride >= 3, -1, "vlb_terms: dst_stride must be >= 3");
  MI355_REQUIRE(offset % 4 == 0, -1, "vlb_terms: the Philox offset must be a multiple of 4");
  MI355_REQUIRE(std::isfinite(st.c_recip) && std::isfinite(st.c_recipm1) && std::isfinite(st.coef1) && std::isfinite(st.coef2), -1,
                "vlb_terms: c_recip, c_recipm1, coef1 and coef2 must be finite");
  MI355_REQUIRE(std::isfinite(st.true_log), -1, "vlb_terms: true_log must be finite");
  if (st.learned) MI355_REQUIRE(std::isfinite(st.min_log) && std::isfinite(st.max_log), -1, "vlb_terms: min_log and max_log must be finite");
  else MI355_REQUIRE(std::isfinite(st.model_log), -1, "vlb_terms: model_log must be finite");
  if (batch == 0) return 0;
  MI355_REQUIRE(x0 && xk && out && dst, -1, "vlb_terms: null argument");
  MI355_REQUIRE(z || use_philox, -1, "vlb_terms: the step's draw is needed (z, or Philox at (seed, offset))");
  const VlbScalars c{(double)st.c_recip, (double)st.c_recipm1, (double)st.coef1, (double)st.coef2,
                     (double)st.true_log, (double)st.model_log, (double)st.min_log, (double)st.max_log, (double)st.sa, (double)st.sb, st.pred};
  const uint64_t off4 = offset / 4;
  const dim3 grid((unsigned)batch), block(256);
  if (!st.k_is_zero)
    hipLaunchKernelGGL((vlb_terms_kernel<false, 0>), grid, block, 0, s, x0, xk, out, out_stride, z, use_philox, seed, off4, c, st.learned, st.clip, dst,
                       dst_stride, per);
  else if (st.cdf == 0)
    hipLaunchKernelGGL((vlb_terms_kernel<true, 0>), grid, block, 0, s, x0, xk, out, out_stride, z, use_philox, seed, off4, c, st.learned, st.clip, dst,
                       dst_stride, per);
  else
    hipLaunchKernelGGL((vlb_terms_kernel<true, 1>), grid, block, 0, s, x0, xk, out, out_stride, z, use_philox, seed, off4, c, st.learned, st.clip, dst,
                       dst_stride, per);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int vlb_prior_launch(const float* x0, float sa_last, float sb_last, const float* terms, int64_t terms_stride, int K, float* summary, int batch,
                     int64_t per, hipStream_t s) {
  MI355_REQUIRE(per > 0, -1, "vlb_prior: elems_per_image must be > 0");
  MI355_REQUIRE(batch >= 0, -1, "vlb_prior: batch must be >= 0");
  MI355_REQUIRE(std::isfinite(sa_last), -1, "vlb_prior: sqrt_alphas_cumprod[K-1] must be finite");
  MI355_REQUIRE(std::isfinite(sb_last) && sb_last > 0.f, -1, "vlb_prior: sqrt_one_minus_alphas_cumprod[K-1] must be finite and > 0");
  MI355_REQUIRE(!terms || (K >= 1 && terms_stride >= 3 * (int64_t)K), -1, "vlb_prior: terms needs K >= 1 and terms_stride >= 3 * K");
  if (batch == 0) return 0;
  MI355_REQUIRE(x0 && summary, -1, "vlb_prior: null argument");
  const double L = 2.0 * std::log((double)sb_last);
  hipLaunchKernelGGL(vlb_prior_kernel, dim3((unsigned)batch), dim3(256), 0, s, x0, (double)sa_last, L, std::exp(L), terms, terms_stride, K, summary, per);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
