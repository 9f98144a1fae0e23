// Per-step sampler updates: HBM-bound fused elementwise kernels over the fp32 NCHW state.
//
// Reference (each is 8-10 separate eager kernels there):
//   Euler update                x += dt*v                  torchdyn fixed-step euler (cifar10/compute_fid.py:79)
//   DDPM ancestral step         sampling.py:59-67 + sde_diffusion.py:220-237
//   Langevin corrector          sampling.py:113-121 + sde_diffusion.py:214-217
//   Replacement mask            sampling.py:225-232 + sde_diffusion.py:239-244
//   clip / uint8 / unit range   sampling.py:13-14, cifar10/compute_fid.py:87, cifar10/utils_cifar.py:40-41
// Noise is either injected (a pre-drawn tensor, for parity with the reference's torch.randn_like
// stream) or generated in-kernel with Philox4x32-10 + Box-Muller keyed by (seed, element index).
#include <cmath>
#include <string>

#include "ops.h"

// torch evaluates a*x - b*e as mul, mul, sub (three roundings); keep that shape so the ill-conditioned
// x0 = c_recip*x - c_recipm1*eps (c ~ 1e3 at high noise levels) tracks the reference bit-for-bit where possible.
#pragma clang fp contract(off)

#include "step_common.h"   // launch_ew4, ld4 / st4, noise4, x0_pre, Pred<K>, ld4_eps, pred_form, ddim_eta_coefs: shared with nullspace.hip

namespace {

// classifier-free guidance of one element: eps_u + w (eps_c - eps_u), the difference, the product and the sum each rounded
__device__ inline float cfg_mix(float ec, float eu, float w) {
  const float d = ec - eu;
  const float p = w * d;
  return eu + p;
}
__device__ inline void cfg_eps4(const float* eps, int64_t nu, float w, const float* w_dev, int64_t per, int64_t stride, int64_t i, int cnt, float (&ev)[4]) {
  float ec[4], eu[4], wv[4] = {w, w, w, w};
  ld4_eps(eps, per, stride, i, cnt, ec); ld4_eps(eps + nu, per, stride, i, cnt, eu);
  if (w_dev) {   // a group of four may straddle images when per % 4 != 0
    int64_t img = i / per, r = i - img * per;
    for (int l = 0; l < cnt; ++l) {
      while (r >= per) { r -= per; ++img; }
      wv[l] = w_dev[img];
      ++r;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) ev[j] = cfg_mix(ec[j], eu[j], wv[j]);
}

// Where a predictor step takes its eps from.  CFG false: eps [n].  CFG true, the classifier-free-guided forms: eps holds 2n values, the conditional
// evaluation in [0, n) and the unconditional one in [n, 2n) (one network call at twice the batch), combined by cfg_eps4; x then holds the duplicated state
// [2n]: the first half is read, the result goes to both halves.  w_dev (optional): one scale per image of `per` elements.
// stride (== per: contiguous): the image stride of eps, so that the unconditional half starts nu = (n / per) * stride floats behind the conditional one.
template <bool CFG> struct EpsSrc {
  const float* eps; int64_t n; float w; const float* w_dev; int64_t per, stride, nu;
  __device__ inline void load(int64_t i, int cnt, float (&ev)[4]) const {
    if constexpr (CFG) cfg_eps4(eps, nu, w, w_dev, per, stride, i, cnt, ev);
    else ld4_eps(eps, per, stride, i, cnt, ev);
  }
  // the learned-variance channels of the (conditional) evaluation: [C, 2C) of each image, at eps + per under the same stride
  __device__ inline void load_v(int64_t i, int cnt, float (&vv)[4]) const { ld4_strided(eps + per, per, stride, i, cnt, vv); }
  __device__ inline void store(float* x, int64_t i, int cnt, const float (&v)[4]) const {
    st4(x, i, cnt, v);
    if constexpr (CFG) st4(x + n, i, cnt, v);
  }
};

// How a predictor step ends its data prediction.  SH false: x0_hat = clip(x0_pre, -1, 1), the reference's process_x0; no row is read.  SH true
// (mi355_x0_shaping): image b of `per` elements has the row shape[b] = (f, s) of x0_shape_stats_kernel; eps is scaled by f (guidance rescale), x0_hat =
// clip(x0_pre, -s, s) / s (dynamic thresholding).  A row (1, 1) gives the static clip's bits: 1 * eps and a division by 1 are exact.
template <bool SH> struct X0Rows {
  const float* shape; int64_t per;
  __device__ inline void load(int64_t i, int cnt, float (&f)[4], float (&s)[4]) const {
    if constexpr (SH) {
#pragma unroll
      for (int l = 0; l < 4; ++l) { f[l] = 1.f; s[l] = 1.f; }
      int64_t img = i / per, r = i - img * per;   // a group of four may straddle images when per % 4 != 0
      for (int l = 0; l < cnt; ++l) {
        while (r >= per) { r -= per; ++img; }
        f[l] = shape[2 * img]; s[l] = shape[2 * img + 1];
        ++r;
      }
    }
  }
  template <class P> __device__ inline float x0(const P& pr, float c_recip, float c_recipm1, float x, float e, float f, float s) const {
    if constexpr (SH) return clip_nan(pr.pre(c_recip, c_recipm1, x, f * e), -s, s) / s;
    else return clip_nan(pr.pre(c_recip, c_recipm1, x, e), -1.f, 1.f);
  }
};
// run f(EpsSrc<CFG>, X0Rows<SH>, Pred<K>) for the form predictor_step_launch was asked for
template <typename F> int step_form(bool cfg, const float* eps, int64_t n, float w, const float* w_dev, int64_t per, int64_t stride, const float* shape, int pred,
                                    float sa, float sb, F&& f) {
  const int64_t nu = stride == per ? n : n / per * stride;
  return pred_form(pred, sa, sb, [&](auto pr) {
    if (cfg) {
      const EpsSrc<true> e{eps, n, w, w_dev, per, stride, nu};
      return shape ? f(e, X0Rows<true>{shape, per}, pr) : f(e, X0Rows<false>{nullptr, 0}, pr);
    }
    const EpsSrc<false> e{eps, n, 0.f, nullptr, per, stride, nu};
    return shape ? f(e, X0Rows<true>{shape, per}, pr) : f(e, X0Rows<false>{nullptr, 0}, pr);
  });
}
}  // namespace

int euler_step_launch(float* x, const float* v, float dt, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float a[4], b[4];
    ld4(x, i, cnt, a); ld4(v, i, cnt, b);
    {
#pragma clang fp contract(off)   // product and sum rounded separately, as `x + dt * v` in eager PyTorch (and as conv_edge.hip's fused form of this step)
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = a[j] + dt * b[j];
    }
    st4(x, i, cnt, a);
  });
}

// Euler-Maruyama step of a diagonal-noise Ito SDE (torchsde's fixed-step Euler: y1 = y0 + f * dt + g * dW), f = ca * a (+ cb * b):
// the SF2M drift is model + score_model (ca = cb = +1), its reverse -model + score_model (ca = -1).  The sum is rounded once before
// the product, as the eager `f` is returned, and y0 + f*dt + g*dW is evaluated left to right with every operation rounded (no
// contraction: this file).  g: per-element tensor or, when null, the scalar g_s.  dW: injected increments, or sqrt(dt) * z with z the
// Philox stream of randn_launch at (seed, offset); neither = no noise.  out (optional): out = x_k + w * (x_{k+1} - x_k), torchsde's linear
// interpolation of an output time inside the step; w == 0 and w == 1 store the end points themselves, as torchsde returns them.
int sde_euler_step_launch(float* x, const float* a, const float* b, float ca, float cb, float dt, const float* g, float g_s, const float* dW,
                          int use_philox, uint64_t seed, uint64_t offset, float* out, float w, int64_t n, hipStream_t s) {
  MI355_REQUIRE(x && a, -1, "sde_euler_step: null argument");
  MI355_REQUIRE(offset % 4 == 0, -1, "sde_euler_step: the Philox offset must be a multiple of 4");
  const uint64_t off4 = offset / 4;
  const float sdt = sqrtf(dt);   // correctly rounded, as torch's fp32 sqrt
  const int noisy = dW != nullptr || use_philox;
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float xv[4], av[4], bv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {g_s, g_s, g_s, g_s}, zz[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(x, i, cnt, xv); ld4(a, i, cnt, av);
    if (b) ld4(b, i, cnt, bv);
    if (g) ld4(g, i, cnt, gv);
    if (noisy) noise4(dW, use_philox, seed, off4, i, i4, cnt, zz);
    float x1[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float f = b ? ca * av[j] + cb * bv[j] : ca * av[j];
      const float dw = dW ? zz[j] : sdt * zz[j];
      x1[j] = noisy ? (xv[j] + f * dt) + gv[j] * dw : xv[j] + f * dt;
    }
    st4(x, i, cnt, x1);
    if (out) {
#pragma unroll
      for (int j = 0; j < 4; ++j) xv[j] = w == 0.f ? xv[j] : (w == 1.f ? x1[j] : xv[j] + w * (x1[j] - xv[j]));
      st4(out, i, cnt, xv);
    }
  });
}

// The predictor steps: one kernel template per kind, all launched by predictor_step_launch (below the last of them).  Each has four forms, chosen by
// step_form: plain or classifier-free-guided (EpsSrc), static clip or per-image shaping (X0Rows).
namespace {
template <class E, class R, class P>
int ddpm_step_form(E es, R rows, P pr, float* x, const float* z, float c_recip, float c_recipm1, float coef1, float coef2, float sigma, int use_philox,
                   uint64_t seed, uint64_t off4, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float xv[4], ev[4], zz[4], fv[4], sv[4];
    ld4(x, i, cnt, xv);
    es.load(i, cnt, ev);
    noise4(z, use_philox, seed, off4, i, i4, cnt, zz);
    rows.load(i, cnt, fv, sv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x0 = rows.x0(pr, c_recip, c_recipm1, xv[j], ev[j], fv[j], sv[j]);   // predict_start_from_noise + process_x0
      const float mean = coef1 * x0 + coef2 * xv[j];                                // q_posterior
      xv[j] = mean + sigma * zz[j];                                                 // exp(0.5*logvar) * noise
    }
    es.store(x, i, cnt, xv);
  });
}
}  // namespace

// The ancestral step of a learned-variance net (Nichol & Dhariwal 2021, eq. 15): the network's second half v interpolates the log-variance between
// max_log = log(beta) and min_log = the clipped posterior log-variance; v is not clamped.  Every operation rounded (no contraction: this file).
namespace {
template <class E, class P>
int ddpm_lv_step_form(E es, P pr, float* x, const float* z, float c_recip, float c_recipm1, float coef1, float coef2, float min_log, float max_log,
                      int use_philox, uint64_t seed, uint64_t off4, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float xv[4], ev[4], vv[4], zz[4];
    ld4(x, i, cnt, xv);
    es.load(i, cnt, ev);
    es.load_v(i, cnt, vv);
    noise4(z, use_philox, seed, off4, i, i4, cnt, zz);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float frac = (vv[j] + 1.f) * 0.5f;
      const float logvar = frac * max_log + (1.f - frac) * min_log;
      const float x0 = clip_nan(pr.pre(c_recip, c_recipm1, xv[j], ev[j]), -1.f, 1.f);
      const float mean = coef1 * x0 + coef2 * xv[j];
      xv[j] = mean + expf(0.5f * logvar) * zz[j];
    }
    es.store(x, i, cnt, xv);
  });
}
}  // namespace

int corrector_step_launch(float* x, const float* eps, const float* z, float c_recip, float c_recipm1, float rsm1, float dt,
                          float delta, int use_philox, uint64_t seed, uint64_t offset, int64_t n, hipStream_t s, int64_t per, int64_t eps_stride, int pred,
                          float sa, float sb) {
  MI355_REQUIRE(offset % 4 == 0, -1, "corrector_step: the Philox offset must be a multiple of 4");
  MI355_REQUIRE(pred >= PRED_EPS && pred <= PRED_V, -1, "corrector_step: the prediction kind must be 0 (eps), 1 (x0) or 2 (v)");
  const int64_t stride = eps_stride ? eps_stride : per;
  MI355_REQUIRE(stride == per || (per > 0 && n % per == 0 && stride > per), -1,
                "corrector_step: an eps stride needs n to be whole images of elems_per_image elements and eps_stride >= elems_per_image");
  const uint64_t off4 = offset / 4;
  const float kd = 0.5f * dt * delta, kn = sqrtf(dt * delta);
  return pred_form(pred, sa, sb, [=](auto pr) {
    return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
      float xv[4], ev[4], zz[4];
      ld4(x, i, cnt, xv); ld4_eps(eps, per, stride, i, cnt, ev);
      noise4(z, use_philox, seed, off4, i, i4, cnt, zz);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = clip_nan(pr.pre(c_recip, c_recipm1, xv[j], ev[j]), -1.f, 1.f);
        const float score = -rsm1 * x0;  // score_from_x0
        xv[j] = xv[j] + (kd * score + kn * zz[j]);
      }
      st4(x, i, cnt, xv);
    });
  });
}

namespace {
template <class E, class R, class P>
int ddim_step_form(E es, R rows, P pr, float* x, float c_recip, float c_recipm1, float sa, float sb, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float xv[4], ev[4], fv[4], sv[4];
    ld4(x, i, cnt, xv);
    es.load(i, cnt, ev);
    rows.load(i, cnt, fv, sv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x0 = rows.x0(pr, c_recip, c_recipm1, xv[j], ev[j], fv[j], sv[j]);
      const float e2 = (c_recip * xv[j] - x0) / c_recipm1;   // the eps that x0_hat stands for: of the clipped (shaped: the thresholded) prediction
      xv[j] = sa * x0 + sb * e2;
    }
    es.store(x, i, cnt, xv);
  });
}
}  // namespace

// DDIM(eta) step (Song et al. 2021, eq. 12) with the reference's clipped x0_hat: the DDIM step's x0 and e2, then
//   x <- sqrt(acp_prev) x0 + sqrt(max(1 - acp_prev - sigma^2, 0)) e2 + sigma z,
// the two square roots taken here on the host (1 - acp_prev - sigma^2 left to right, sigma^2 rounded).  Noise as the ancestral step; with neither z
// nor Philox the noise term is not added at all, so sigma = 0 without noise gives the DDIM step's bits.
namespace {
template <class E, class R, class P>
int ddim_eta_step_form(E es, R rows, P pr, float* x, const float* z, float c_recip, float c_recipm1, float sa, float sb, float sigma, int noisy, int use_philox,
                       uint64_t seed, uint64_t off4, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float xv[4], ev[4], zz[4] = {0.f, 0.f, 0.f, 0.f}, fv[4], sv[4];
    ld4(x, i, cnt, xv);
    es.load(i, cnt, ev);
    if (noisy) noise4(z, use_philox, seed, off4, i, i4, cnt, zz);
    rows.load(i, cnt, fv, sv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x0 = rows.x0(pr, c_recip, c_recipm1, xv[j], ev[j], fv[j], sv[j]);
      const float e2 = (c_recip * xv[j] - x0) / c_recipm1;
      const float m = sa * x0 + sb * e2;
      xv[j] = noisy ? m + sigma * zz[j] : m;
    }
    es.store(x, i, cnt, xv);
  });
}
}  // namespace

// Forward move q(x_k | x_{k-1}) of a (respaced) chain: x <- a x + b z with a = sqrt(alphas_k), b = sqrt(betas_k), two rounded products and one
// sum.  Noise as the ancestral step (neither z nor Philox: z = 0, x <- a x + b * 0).
int renoise_step_launch(float* x, const float* z, float a, float b, int use_philox, uint64_t seed, uint64_t offset, int64_t n, hipStream_t s) {
  MI355_REQUIRE(offset % 4 == 0, -1, "renoise_step: the Philox offset must be a multiple of 4");
  MI355_REQUIRE(n <= 0 || x, -1, "renoise_step: null argument");
  const uint64_t off4 = offset / 4;
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float xv[4], zz[4];
    ld4(x, i, cnt, xv);
    noise4(z, use_philox, seed, off4, i, i4, cnt, zz);
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[j] = a * xv[j] + b * zz[j];
    st4(x, i, cnt, xv);
  });
}

// The forward marginal q(x_k | x_0) out of place: out = a x0 + b z with a = sqrt_alphas_cumprod[k], b = sqrt_one_minus_alphas_cumprod[k], two rounded
// products and one sum (the bits of lincomb_per_sample_launch on the same operands); x0 is left as it is.  Noise as the ancestral step.
int q_sample_launch(float* out, const float* x0, const float* z, float a, float b, int use_philox, uint64_t seed, uint64_t offset, int64_t n,
                    hipStream_t s) {
  MI355_REQUIRE(offset % 4 == 0, -1, "q_sample: the Philox offset must be a multiple of 4");
  MI355_REQUIRE(n <= 0 || (out && x0), -1, "q_sample: null argument");
  MI355_REQUIRE(out != x0 || n <= 0, -1, "q_sample: out must not be x0 (renoise_step is the in-place move)");
  const uint64_t off4 = offset / 4;
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float xv[4], zz[4], o[4];
    ld4(x0, i, cnt, xv);
    noise4(z, use_philox, seed, off4, i, i4, cnt, zz);
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = a * xv[j] + b * zz[j];
    st4(out, i, cnt, o);
  });
}

int replace_mask_launch(float* x, const float* cond, const float* z, float pad, int noisy, float sa, float sb, int use_philox,
                        uint64_t seed, uint64_t offset, int64_t n, hipStream_t s) {
  MI355_REQUIRE(offset % 4 == 0, -1, "replace_mask: the Philox offset must be a multiple of 4");
  const uint64_t off4 = offset / 4;
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float xv[4], cv[4], zz[4] = {0.f, 0.f, 0.f, 0.f};
    ld4(x, i, cnt, xv); ld4(cond, i, cnt, cv);
    if (noisy) noise4(z, use_philox, seed, off4, i, i4, cnt, zz);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float nc = noisy ? sa * cv[j] + sb * zz[j] : cv[j];  // q_sample(condition, i)
      xv[j] = cv[j] == pad ? xv[j] : nc;                         // torch.where(condition == pad_value, xi, noised)
    }
    st4(x, i, cnt, xv);
  });
}

int clip_launch(float* x, float lo, float hi, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float a[4];
    ld4(x, i, cnt, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = clip_nan(a[j], lo, hi);
    st4(x, i, cnt, a);
  });
}

// Per-sample mean squared error, torch.mean((a - b)**2, dim=(1, 2, 3)) of the evaluation loop (AD/experiments/main.py:299):
// one workgroup per sample, fp32 differences, fp64 accumulation.
__global__ void __launch_bounds__(256) mse_per_sample_kernel(const float* a, const float* b, float* out, int64_t per) {
  __shared__ double sh[4];
  const float* pa = a + (int64_t)blockIdx.x * per;
  const float* pb = b + (int64_t)blockIdx.x * per;
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < per; i += 256) { const float d = pa[i] - pb[i]; acc += (double)d * (double)d; }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) out[blockIdx.x] = (float)((sh[0] + sh[1] + sh[2] + sh[3]) / (double)per);
}
int mse_per_sample_launch(const float* a, const float* b, float* out, int batch, int64_t per, hipStream_t s) {
  MI355_REQUIRE(batch > 0 && per > 0, -2, "mse_per_sample: empty input");
  hipLaunchKernelGGL(mse_per_sample_kernel, dim3((unsigned)batch), dim3(256), 0, s, a, b, out, per);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

// Per-image drift of a cached feature between two full evaluations (feature reuse across sampler steps, mi355_feature_cache::drift_out):
//   out[b] = ||cur_b - prev_b||^2 / ||prev_b||^2,  then prev_b <- cur_b,
// cur and prev [batch][per] in the plan's element type, read once each; the copy rides in the same pass.  Bandwidth-bound: one 512-thread
// workgroup per image, 16-byte loads and stores, four fragments of each tensor in flight per thread; sums in fp32, one accumulator per
// fragment element (a thread's chain is per / (512 * VEC) terms long), then the wave shuffle and eight LDS partials.  Every (image, fragment)
// is read and written by one thread, in a fixed order: no atomics, bitwise reproducible.  prev == 0 everywhere: IEEE (inf, or NaN for 0 / 0).
template <typename T>
__global__ void __launch_bounds__(512) feature_drift_kernel(const T* __restrict__ cur, T* __restrict__ prev, float* out, int64_t per) {
  constexpr int V = Elem<T>::VEC;
  __shared__ float sh[2][8];
  const u32x4* pc = reinterpret_cast<const u32x4*>(cur + (int64_t)blockIdx.x * per);
  u32x4* pp = reinterpret_cast<u32x4*>(prev + (int64_t)blockIdx.x * per);
  const int64_t nv = per / V;
  float num[V], den[V];
#pragma unroll
  for (int j = 0; j < V; ++j) num[j] = den[j] = 0.f;
  for (int64_t i0 = threadIdx.x; i0 < nv; i0 += 4 * 512) {
    u32x4 c[4], p[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = i0 + u * 512;
      if (i < nv) { c[u] = pc[i]; p[u] = pp[i]; }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t i = i0 + u * 512;
      if (i >= nv) continue;
      float fc[V], fp[V];
      frag_to_float(c[u], fc, T()); frag_to_float(p[u], fp, T());
#pragma unroll
      for (int j = 0; j < V; ++j) { const float d = fc[j] - fp[j]; num[j] += d * d; den[j] += fp[j] * fp[j]; }
      pp[i] = c[u];
    }
  }
  float n = 0.f, d = 0.f;
#pragma unroll
  for (int j = 0; j < V; ++j) { n += num[j]; d += den[j]; }
  for (int o = 32; o > 0; o >>= 1) { n += __shfl_xor(n, o); d += __shfl_xor(d, o); }
  if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = n; sh[1][threadIdx.x >> 6] = d; }
  __syncthreads();
  if (threadIdx.x == 0) {
    n = d = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) { n += sh[0][w]; d += sh[1][w]; }
    out[blockIdx.x] = n / d;
  }
}
int feature_drift_launch(int dtype, const void* cur, void* prev, int batch, int64_t per, float* out, hipStream_t s) {
  MI355_REQUIRE(cur && prev && out, -1, "feature_drift: null argument");
  MI355_REQUIRE(cur != prev, -1, "feature_drift: cur and prev must be different buffers");
  MI355_REQUIRE(batch > 0, -1, "feature_drift: batch must be positive");
  const int vec = dtype == DT_F32 ? 4 : 8;
  MI355_REQUIRE(per > 0 && per % vec == 0, -2, "feature_drift: elems_per_image must be a positive multiple of 16 bytes of elements");
  MI355_REQUIRE(((reinterpret_cast<uintptr_t>(cur) | reinterpret_cast<uintptr_t>(prev)) & 15) == 0, -2, "feature_drift: cur and prev must be 16-byte aligned");
  return dispatch_dtype(dtype, [&](auto tag) -> int {
    using T = decltype(tag);
    hipLaunchKernelGGL(feature_drift_kernel<T>, dim3((unsigned)batch), dim3(512), 0, s, reinterpret_cast<const T*>(cur), reinterpret_cast<T*>(prev), out, per);
    MI355_CHECK_HIP(hipGetLastError());
    return 0;
  });
}

// EMA of a parameter tensor: target = target * decay + source * (1 - decay)  (cifar10/utils_cifar.py:47-53), two separately
// rounded products like the reference's eager expression (this file is compiled with fp contraction off).
int ema_update_launch(float* target, const float* source, float decay, float one_minus_decay, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float t[4], v[4];
    ld4(target, i, cnt, t);
    ld4(source, i, cnt, v);
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = t[j] * decay + v[j] * one_minus_decay;
    st4(target, i, cnt, t);
  });
}

int quantize_u8_launch(const float* x, uint8_t* out, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float a[4];
    ld4(x, i, cnt, a);
    uint8_t q[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float v = clip_nan(a[j] * 127.5f + 128.f, 0.f, 255.f);
      q[j] = (uint8_t)(int)v;  // .to(uint8): truncation toward zero
    }
    if (cnt == 4 && ((reinterpret_cast<uintptr_t>(out + i) & 3) == 0)) {
      *reinterpret_cast<uint32_t*>(out + i) = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
    } else {
      for (int j = 0; j < cnt; ++j) out[i + j] = q[j];
    }
  });
}

int to_unit_range_launch(const float* x, float* out, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float a[4];
    ld4(x, i, cnt, a);
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] = clip_nan(a[j], -1.f, 1.f) / 2.f + 0.5f;
    st4(out, i, cnt, a);
  });
}

int randn_launch(float* out, uint64_t seed, uint64_t offset, int64_t n, hipStream_t s) {
  MI355_REQUIRE(offset % 4 == 0, -1, "randn: the Philox offset must be a multiple of 4");
  const uint64_t off4 = offset / 4;
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float zz[4];
    randn4(seed, off4 + (uint64_t)i4, zz);
    st4(out, i, cnt, zz);
  });
}

int fill_launch(float* x, float v, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float a[4] = {v, v, v, v};
    st4(x, i, cnt, a);
  });
}

// out[n, :] = a[n] * x[n, :] + b[n] * y[n, :] with per-sample coefficients (device arrays gathered from the DDPM tables by
// `extract`, sde_diffusion.py:101-104): predict_start_from_noise / q_posterior mean / q_sample / score_from_x0
// (sde_diffusion.py:214-244).  Two separately rounded products and one add, like the reference's eager expression; y (and b)
// may be null (out = a * x).  `per` = elements per sample.
int lincomb_per_sample_launch(float* out, const float* x, const float* y, const float* a, const float* b, int batch, int64_t per,
                              hipStream_t s) {
  MI355_REQUIRE(out && x && a && batch > 0 && per > 0, -1, "lincomb_per_sample: bad argument");
  MI355_REQUIRE((y == nullptr) == (b == nullptr), -1, "lincomb_per_sample: y and b go together");
  const int64_t n = (int64_t)batch * per;
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float xv[4], yv[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    ld4(x, i, cnt, xv);
    if (y) ld4(y, i, cnt, yv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int64_t smp = (i + j) / per;   // a 4-element group may straddle two samples when per % 4 != 0
      const int64_t sc = smp < batch ? smp : batch - 1;
      o[j] = y ? a[sc] * xv[j] + b[sc] * yv[j] : a[sc] * xv[j];
    }
    st4(out, i, cnt, o);
  });
}

namespace {
// ---- condition builders (once per batch / once per solve; AD/image_diffusion/likelihoods.py, mnist/utils_mnist_hy.py:18-28) ----------
// Bilinear resize of NCHW fp32 planes, align_corners = False, no antialiasing: torch.nn.functional.interpolate(mode="bilinear")
// as the reference calls it for the low-res condition (downsample_images, HyperResolution._sample, the SuperRes wrapper's
// upsampling).  Source index = scale * (dst + 0.5) - 0.5 clamped at 0, scale = in / out in fp32; the four taps are combined as
// h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11), the operation order of ATen's kernel (no fused multiply-adds here).
__global__ void __launch_bounds__(256) resize_bilinear_kernel(const float* in, float* out, int64_t planes, int Hi, int Wi, int Ho, int Wo,
                                                               float sh, float sw) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= planes * Ho * Wo) return;
  const int ox = (int)(idx % Wo);
  const int oy = (int)((idx / Wo) % Ho);
  const int64_t pl = idx / ((int64_t)Wo * Ho);
  float fy = sh * ((float)oy + 0.5f) - 0.5f; fy = fy < 0.f ? 0.f : fy;
  float fx = sw * ((float)ox + 0.5f) - 0.5f; fx = fx < 0.f ? 0.f : fx;
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < Hi - 1 ? 1 : 0), x1 = x0 + (x0 < Wi - 1 ? 1 : 0);
  const float h1 = fminf(fmaxf(fy - (float)y0, 0.f), 1.f), w1 = fminf(fmaxf(fx - (float)x0, 0.f), 1.f);
  const float h0 = 1.f - h1, w0 = 1.f - w1;
  const float* p = in + pl * (int64_t)Hi * Wi;
  const float v00 = p[(int64_t)y0 * Wi + x0], v01 = p[(int64_t)y0 * Wi + x1], v10 = p[(int64_t)y1 * Wi + x0], v11 = p[(int64_t)y1 * Wi + x1];
  out[idx] = h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11);
}

// InPainting._sample / OutPainting._sample (likelihoods.py:78-87, 95-104) for a whole batch in one launch: image n's square patch
// has its top-left corner at (top[n], left[n]) (drawn on the host in the reference's order); inside the patch the result is
// pad_value (in-painting) or the image (out-painting), outside it the other one.
__global__ void __launch_bounds__(256) paint_patch_kernel(const float* img, const int* top, const int* left, int patch, float pad,
                                                           int outpaint, float* out, int64_t n_elems, int C, int H, int W) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= n_elems) return;
  const int x = (int)(idx % W), y = (int)((idx / W) % H);
  const int64_t n = idx / ((int64_t)W * H * C);
  const int t = top[n], l = left[n];
  const bool inside = y >= t && y < t + patch && x >= l && x < l + patch;
  out[idx] = (inside != (outpaint != 0)) ? pad : img[idx];
}

}  // namespace

int resize_bilinear_launch(const float* in, float* out, int64_t planes, int Hi, int Wi, int Ho, int Wo, hipStream_t s) {
  MI355_REQUIRE(in && out && planes > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, -1, "resize_bilinear: bad argument");
  const int64_t n = planes * Ho * Wo;
  hipLaunchKernelGGL(resize_bilinear_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in, out, planes, Hi, Wi, Ho, Wo,
                     (float)Hi / (float)Ho, (float)Wi / (float)Wo);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int paint_patch_launch(const float* img, const int* top, const int* left, int patch, float pad, int outpaint, float* out, int N, int C,
                       int H, int W, hipStream_t s) {
  MI355_REQUIRE(img && top && left && out && N > 0 && C > 0 && H > 0 && W > 0 && patch > 0, -1, "paint_patch: bad argument");
  const int64_t n = (int64_t)N * C * H * W;
  hipLaunchKernelGGL(paint_patch_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, img, top, left, patch, pad, outpaint, out, n, C, H, W);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

// DPM-Solver++ multistep step (Lu et al. 2022, Algorithm 2) in the data-prediction form, on the clipped x0_hat of every step above:
//   D = clip(c_recip x - c_recipm1 eps, -1, 1);   x <- cx x + c0 D + c1 hist;   hist <- D
// evaluated as ((cx x) + (c0 D)) + (c1 hist), every product and sum rounded (8 roundings with D's three).  c1 == 0 (order 1, the first step run,
// the last one): hist is not read and the sum ends at the second term, so an uninitialised history never reaches the state.  hist == null: D is
// not kept.  The host coefficients are DDPM.dpm_solver_coefs.
// With shaping rows D is the shaped x0_hat, and that is what the history keeps.
namespace {
template <class E, class R, class P>
int dpmpp_step_form(E es, R rows, P pr, float* x, float* hist, float c_recip, float c_recipm1, float cx, float c0, float c1, int64_t n, hipStream_t s) {
  const bool two = c1 != 0.f;
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t, int cnt) {
    float xv[4], ev[4], hv[4] = {0.f, 0.f, 0.f, 0.f}, dv[4], fv[4], sv[4];
    ld4(x, i, cnt, xv);
    es.load(i, cnt, ev);
    if (two) ld4(hist, i, cnt, hv);
    rows.load(i, cnt, fv, sv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float d = rows.x0(pr, c_recip, c_recipm1, xv[j], ev[j], fv[j], sv[j]);
      const float m = cx * xv[j] + c0 * d;
      xv[j] = two ? m + c1 * hv[j] : m;
      dv[j] = d;
    }
    es.store(x, i, cnt, xv);
    if (hist) st4(hist, i, cnt, dv);
  });
}
}  // namespace

// The one launcher of the four predictor steps (PredictorStep, ops.h): every refusal once, prefixed by the name of the form asked for, then the host
// side of the kind's coefficients, then the kernel template of the kind in the form step_form picks.
int predictor_step_launch(const PredictorStep& p, hipStream_t s) {
  static const char* const names[5][2] = {{"ddpm_step", "ddpm_cfg_step"}, {"ddim_step", "ddim_cfg_step"}, {"ddim_eta_step", "ddim_eta_cfg_step"},
                                          {"dpmpp_step", "dpmpp_cfg_step"}, {"ddpm_lv_step", "ddpm_lv_cfg_step"}};
  const bool cfg = p.guide.on;
  const auto f = [&] { return std::string(names[p.kind][cfg]) + ": "; };   // built inside a refusal only: MI355_REQUIRE evaluates its message on failure
  float* const x = p.x; const float* const eps = p.eps; const float* const z = p.z; float* const hist = p.hist;
  const float* const w_dev = cfg ? p.guide.w_dev : nullptr; const float* const shape = p.shape;
  const float c_recip = p.c_recip, c_recipm1 = p.c_recipm1, sigma = p.sigma, c1 = p.c;
  const int use_philox = p.use_philox;
  const uint64_t seed = p.seed, offset = p.offset;
  const int64_t per = p.per, n = p.n;
  const int64_t stride = p.eps_stride ? p.eps_stride : per;   // == per: the contiguous read
  const bool draws = p.kind == STEP_ANCESTRAL || p.kind == STEP_DDIM_ETA || p.kind == STEP_ANCESTRAL_LV;   // the kinds with a noise term: the others never read the noise triple
  if (draws) MI355_REQUIRE(offset % 4 == 0, -1, f() + "the Philox offset must be a multiple of 4");
  MI355_REQUIRE(!w_dev || (per > 0 && n % per == 0), -1, f() + "per-image scales need n to be whole images of elems_per_image elements");
  MI355_REQUIRE(n <= 0 || (x && eps), -1, f() + "null argument");
  MI355_REQUIRE(p.pred >= PRED_EPS && p.pred <= PRED_V, -1, f() + "the prediction kind must be 0 (eps), 1 (x0) or 2 (v)");
  if (p.kind == STEP_DDIM_ETA) MI355_REQUIRE(sigma >= 0.f && sigma <= 3.0e38f, -1, f() + "sigma must be finite and >= 0");
  if (p.kind == STEP_DPMPP) MI355_REQUIRE(c1 == 0.f || hist || n <= 0, -1, f() + "c1 != 0 needs hist (the previous step's data prediction)");
  MI355_REQUIRE(!shape || (per > 0 && n % per == 0), -1, f() + "per-image shaping rows need n to be whole images of elems_per_image elements");
  MI355_REQUIRE(stride == per || (per > 0 && n % per == 0 && stride > per), -1,
                f() + "an eps stride needs n to be whole images of elems_per_image elements and eps_stride >= elems_per_image");
  MI355_REQUIRE(stride == per || !shape, -1, f() + "per-image shaping rows are not built for a strided eps");
  if (p.kind == STEP_ANCESTRAL_LV) {
    MI355_REQUIRE(!shape, -1, f() + "per-image shaping rows are not built for the learned-variance step");
    MI355_REQUIRE(per > 0 && n % per == 0 && stride >= 2 * per, -1,
                  f() + "the variance channels sit behind the eps channels of each image: eps_stride >= 2 * elems_per_image, n whole images");
    MI355_REQUIRE(std::isfinite(p.min_log) && std::isfinite(p.max_log), -1, f() + "min_log and max_log must be finite");
  }
  const uint64_t off4 = offset / 4;
  if (p.kind == STEP_ANCESTRAL_LV) {
    const float min_log = p.min_log, max_log = p.max_log;
    return step_form(cfg, eps, n, p.guide.w, w_dev, per, stride, nullptr, p.pred, p.sa, p.sb, [=](auto es, auto, auto pr) {
      return ddpm_lv_step_form(es, pr, x, z, c_recip, c_recipm1, p.a, p.b, min_log, max_log, use_philox, seed, off4, n, s);
    });
  }
  return step_form(cfg, eps, n, p.guide.w, w_dev, per, stride, shape, p.pred, p.sa, p.sb, [=](auto es, auto rows, auto pr) {
    switch (p.kind) {
      case STEP_ANCESTRAL:
        return ddpm_step_form(es, rows, pr, x, z, c_recip, c_recipm1, p.a, p.b, sigma, use_philox, seed, off4, n, s);
      case STEP_DDIM:
        return ddim_step_form(es, rows, pr, x, c_recip, c_recipm1, sqrtf(p.a), sqrtf(1.0f - p.a), n, s);
      case STEP_DDIM_ETA: {
        const DdimEta c = ddim_eta_coefs(p.a, sigma);
        const int noisy = z != nullptr || use_philox;
        return ddim_eta_step_form(es, rows, pr, x, z, c_recip, c_recipm1, c.sa, c.sb, sigma, noisy, use_philox, seed, off4, n, s);
      }
      default:
        return dpmpp_step_form(es, rows, pr, x, hist, c_recip, c_recipm1, p.a, p.b, c1, n, s);
    }
  });
}

// ---- per-image statistics of a predictor step's data prediction (mi355_x0_shaping) -------------------------------------------------------------------
// One workgroup per image, no communication between workgroups, no global atomics.  For image b of `per` elements, with eps_g the plain eps or
// cfg_mix of the two halves (w, or w_dev[b]):
//   guidance rescale (Lin et al. 2023, section 3.4): sigma_c, sigma_g = the population standard deviations of eps_c and eps_g over the image (mean first,
//     then the centred sum of squares, fp32, in the fixed order of block_sum2), f = phi * (sigma_c / sigma_g) + (1 - phi); f = 1 when sigma_g == 0;
//   dynamic thresholding (Saharia et al. 2022, section 2.3): lo, hi = the k-th and min(k + 1, per - 1)-th smallest of |x0_pre(x, f * eps_g)|,
//     s_raw = lo + frac * (hi - lo) (torch.quantile's linear interpolation), s = min(max(s_raw, 1), s_max); an image with a NaN gets s = NaN.
// The selection is exact: a radix select over the bit patterns of |x0| (non-negative floats order as their uint32; the sign bit is cleared, so -0 is
// +0), four passes of 8 bits from the top, each a 256-bin histogram in LDS (one per wave, to spread the ds_add traffic) of the keys that carry the
// prefix chosen so far, then a scan of the bins for the one that holds the rank.  Every pass recomputes x0 from x and eps, which sit in L2 behind
// the evaluation that wrote them: one code path for every image size (a 3 x 128 x 128 image is 192 KiB, more than a CU's LDS).  A bin index is
// (key >> shift) & 255 and a rank is < per, so a NaN or an infinity indexes nothing out of range and no loop depends on the data.
namespace {
constexpr int XS_THREADS = 1024, XS_WAVES = XS_THREADS / 64;
struct X0StatsArgs {
  const float* x; const float* eps; const float* w_dev; float* shape; float* detail;
  int64_t n, per, k;
  float w, c_recip, c_recipm1, phi, one_minus_phi, frac, s_max;
  int guided, do_var, do_sel;
  int pred;   // PRED_*: x0_pre of the kind; c_recip, c_recipm1 then hold sa, sb for v and are not read for x0 (nor is x)
};

__global__ void __launch_bounds__(XS_THREADS) x0_shape_stats_kernel(X0StatsArgs a) {
  __shared__ uint32_t hist[XS_WAVES][256];
  __shared__ float redf[2][XS_WAVES];
  __shared__ uint32_t redu[XS_WAVES];
  __shared__ uint32_t sel[4];
  __shared__ uint32_t any_nan;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x, per = a.per;
  const float* xp = a.x + b * per;
  const float* ec = a.eps + b * per;
  const float* eu = ec + a.n;   // read only when guided
  const float w = a.w_dev ? a.w_dev[b] : a.w;
  const bool guided = a.guided != 0;
  auto eps_g = [&](int64_t j) { return guided ? cfg_mix(ec[j], eu[j], w) : ec[j]; };
  // sums of p and q over the workgroup, the same value in every thread: butterfly inside a wave, then the waves in order
  auto block_sum2 = [&](float& p, float& q) {
    for (int o = 32; o > 0; o >>= 1) { p += __shfl_xor(p, o); q += __shfl_xor(q, o); }
    __syncthreads();
    if (lane == 0) { redf[0][wv] = p; redf[1][wv] = q; }
    __syncthreads();
    p = 0.f; q = 0.f;
    for (int i = 0; i < XS_WAVES; ++i) { p += redf[0][i]; q += redf[1][i]; }
  };

  float f = 1.f, sig_c = 0.f, sig_g = 0.f;
  if (a.do_var) {
    float sc = 0.f, sg = 0.f;
    for (int64_t j = tid; j < per; j += XS_THREADS) { sc += ec[j]; sg += eps_g(j); }
    block_sum2(sc, sg);
    const float mc = sc / (float)per, mg = sg / (float)per;
    float qc = 0.f, qg = 0.f;
    for (int64_t j = tid; j < per; j += XS_THREADS) {
      const float dc = ec[j] - mc, dg = eps_g(j) - mg;
      qc += dc * dc; qg += dg * dg;
    }
    block_sum2(qc, qg);
    sig_c = sqrtf(qc / (float)per); sig_g = sqrtf(qg / (float)per);
    if (a.phi != 0.f && sig_g != 0.f) f = a.phi * (sig_c / sig_g) + a.one_minus_phi;
  }

  float s = 1.f, s_raw = 0.f;
  if (a.do_sel) {
    const bool reads_x = a.pred != PRED_X0;   // uniform over the launch
    auto key_of = [&](int64_t j) {
      const float fe = f * eps_g(j);
      return __float_as_uint(reads_x ? x0_pre(a.c_recip, a.c_recipm1, xp[j], fe) : fe) & 0x7fffffffu;
    };
    uint32_t prefix = 0, rank = (uint32_t)a.k, eq = 0, saw_nan = 0;
    if (tid == 0) any_nan = 0;
    for (int pass = 0; pass < 4; ++pass) {
      const int shift = 24 - 8 * pass;
      const uint32_t mask = pass == 0 ? 0u : 0xffffffffu << (shift + 8);
      for (int t = tid; t < XS_WAVES * 256; t += XS_THREADS) (&hist[0][0])[t] = 0;
      __syncthreads();
      for (int64_t j = tid; j < per; j += XS_THREADS) {
        const uint32_t key = key_of(j);
        saw_nan |= key > 0x7f800000u;
        if ((key & mask) == prefix) atomicAdd(&hist[wv][(key >> shift) & 255u], 1u);
      }
      __syncthreads();
      uint32_t c = 0, incl = 0;
      if (tid < 256) {   // bin tid: its count over the waves, then an inclusive scan over the 256 bins (waves 0..3 whole)
        for (int i = 0; i < XS_WAVES; ++i) c += hist[i][tid];
        incl = c;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if (lane >= o) incl += v; }
        if (lane == 63) redu[wv] = incl;
      }
      __syncthreads();
      if (tid < 256) {
        for (int i = 0; i < wv; ++i) incl += redu[i];
        const uint32_t excl = incl - c;
        if (rank >= excl && rank < incl) { sel[0] = (uint32_t)tid; sel[1] = rank - excl; sel[2] = c; }   // exactly one bin: rank < the keys counted
      }
      __syncthreads();
      prefix |= sel[0] << shift; rank = sel[1]; eq = sel[2];
    }
    // prefix is the k-th smallest key, one of `eq` equal keys, and the k-th is number `rank` among them.  The next one in order is the same value, or
    // the smallest key above it; none above (k = per - 1): min(k + 1, per - 1) = k.
    uint32_t mn = 0xffffffffu;
    for (int64_t j = tid; j < per; j += XS_THREADS) { const uint32_t key = key_of(j); if (key > prefix && key < mn) mn = key; }
    for (int o = 32; o > 0; o >>= 1) { const uint32_t v = __shfl_xor(mn, o); mn = v < mn ? v : mn; }
    if (saw_nan) any_nan = 1;
    if (lane == 0) redu[wv] = mn;   // the scan's last read of redu lies before the loop's last barrier
    __syncthreads();
    for (int i = 0; i < XS_WAVES; ++i) mn = redu[i] < mn ? redu[i] : mn;
    const uint32_t hi_key = (rank + 1 < eq || mn == 0xffffffffu) ? prefix : mn;
    const float lo = __uint_as_float(prefix), hi = __uint_as_float(hi_key);
    const float d = hi - lo;
    const float t = a.frac * d;
    s_raw = any_nan ? __builtin_nanf("") : lo + t;
    s = s_raw != s_raw ? s_raw : (s_raw < 1.f ? 1.f : s_raw);
    if (a.s_max > 0.f && s > a.s_max) s = a.s_max;
  }
  if (tid == 0) {
    a.shape[2 * b] = f; a.shape[2 * b + 1] = s;
    if (a.detail) { float* dt = a.detail + 4 * b; dt[0] = sig_c; dt[1] = sig_g; dt[2] = s_raw; dt[3] = 0.f; }
  }
}
}  // namespace

int check_x0_shaping(const char* who, const mi355_x0_shaping* sh, int guided) {
  if (!sh) return 0;
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(sh->quantile >= 0.f && sh->quantile <= 1.f, -1, f + "shaping->quantile must be finite and in [0, 1] (0: thresholding off)");
  MI355_REQUIRE(sh->max_threshold == 0.f || sh->max_threshold >= 1.f, -1, f + "shaping->max_threshold must be 0 (no cap) or >= 1");
  MI355_REQUIRE(sh->rescale_phi >= 0.f && sh->rescale_phi <= 1.f, -1, f + "shaping->rescale_phi must be in [0, 1]");
  MI355_REQUIRE(sh->rescale_phi == 0.f || guided, -1,
                f + "shaping->rescale_phi > 0 needs guided != 0 (the rescale compares the guided eps with the conditional one)");
  return 0;
}

int x0_shape_stats_launch(const float* x, const float* eps, const StepGuide& g, float c_recip, float c_recipm1, const mi355_x0_shaping* sh, float* shape,
                          float* detail, int batch, int64_t per, hipStream_t s, int pred, float sa, float sb) {
  const int guided = g.on;
  if (int rc = check_x0_shaping("x0_shape_stats", sh, guided)) return rc;
  MI355_REQUIRE(pred >= PRED_EPS && pred <= PRED_V, -1, "x0_shape_stats: the prediction kind must be 0 (eps), 1 (x0) or 2 (v)");
  MI355_REQUIRE(x || pred == PRED_X0, -1, "x0_shape_stats: x is null");
  MI355_REQUIRE(eps, -1, "x0_shape_stats: eps is null");
  MI355_REQUIRE(shape, -1, "x0_shape_stats: shape is null");
  MI355_REQUIRE(batch > 0, -1, "x0_shape_stats: batch must be > 0");
  MI355_REQUIRE(per > 0 && per <= ((int64_t)1 << 30), -1, "x0_shape_stats: elems_per_image must be in [1, 2^30]");
  X0StatsArgs a = {};
  a.x = x; a.eps = eps; a.w_dev = guided ? g.w_dev : nullptr; a.shape = shape; a.detail = detail;
  a.n = (int64_t)batch * per; a.per = per;
  a.w = g.w; a.c_recip = pred == PRED_V ? sa : c_recip; a.c_recipm1 = pred == PRED_V ? sb : c_recipm1;
  a.guided = guided; a.pred = pred;
  const float q = sh ? sh->quantile : 0.f, phi = sh ? sh->rescale_phi : 0.f;
  a.phi = phi; a.one_minus_phi = 1.0f - phi;
  a.s_max = sh ? sh->max_threshold : 0.f;
  a.do_var = phi != 0.f || detail != nullptr;
  a.do_sel = q > 0.f;
  if (a.do_sel) {   // torch.quantile's position: q (per - 1) in double, its floor and its fraction
    const double pos = (double)q * (double)(per - 1);
    a.k = (int64_t)std::floor(pos);
    if (a.k > per - 1) a.k = per - 1;
    a.frac = (float)(pos - (double)a.k);
  }
  hipLaunchKernelGGL(x0_shape_stats_kernel, dim3((unsigned)batch), dim3(XS_THREADS), 0, s, a);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

