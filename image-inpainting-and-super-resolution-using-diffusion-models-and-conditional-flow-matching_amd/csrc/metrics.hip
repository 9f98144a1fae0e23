// Per-sample image quality of a reconstruction against its ground truth: MSE, data range, PSNR and SSIM from one launch.
//
// Reference (a Python loop over the batch, one device-to-host copy and two skimage calls per image):
//   calculate_psnr / calculate_ssim     AD/image_diffusion/trainer2.py:15-30, called per image at trainer2.py:119-121
//   skimage.metrics.peak_signal_noise_ratio(x, ref, data_range = ref.max() - ref.min())
//   skimage.metrics.structural_similarity(x, ref, channel_axis = 0, data_range = ref.max() - ref.min())
// SSIM is evaluated at the window positions that lie wholly inside the image (skimage's crop of (win - 1) / 2 pixels), so no border
// mode is involved.  Every product, window sum, S and the means are fp64 (a product of two fp32 values is exact there): in fp32 the
// cancellation in uxx - ux * ux costs 8.5e-7 relative on a smooth pair, 14 fp32 rounding units.  Each output is rounded to fp32 once.
#include "ops.h"

// S(x, x) is exactly 1 only if 2*ux*uy, ux*ux + uy*uy and the three (co)variances are rounded operation by operation in the shape
// they are written in below; a fused multiply-add in one of them and not in its twin breaks that.
#pragma clang fp contract(off)

namespace {

// Tile geometry.  One 256-thread workgroup owns a sample and walks its channels in tiles of TH x TW OUTPUT positions (window
// centres), rows in bands of TH, columns in tiles of TW, so the LDS need is independent of H and W:
//   sx, sy : the (TH + win - 1) x (TW + win - 1) input patch of both images, fp32, row stride IC_MAX floats      2 * 30 * 46 * 4 B = 11040 B
//   hs     : five planes (x, y, xx, yy, xy) of (TH + win - 1) x TW horizontal window sums, fp64, row stride TW    5 * 30 * 32 * 8 B = 38400 B
// at win = 15, the largest window.  A plane row is TW = 32 doubles = 256 B = one LDS bank row.  Both the horizontal pass (writes) and the
// vertical pass (reads) give consecutive lanes consecutive columns of ONE row, a wave's 32-lane half covers a whole plane row and the
// other half the next one: 8-byte reads (bank = dword address mod 64, conflicts within a 32-lane half) touch every bank once per half,
// 8-byte writes (16-lane groups, bank mod 32) cover 32 consecutive dwords per group.  No lane group ever walks down a column, so the
// power-of-two stride needs no padding.  The fp32 patch is read as sx[r][c + k] with c consecutive over lanes: conflict-free as well.
constexpr int MAX_WIN = 15;
constexpr int TH = 16, TW = 32;
constexpr int IR_MAX = TH + MAX_WIN - 1, IC_MAX = TW + MAX_WIN - 1;

struct Taps { float t[MAX_WIN]; };

// UNIFORM: the window is 1 / win^2 everywhere; the sums are unweighted (exact products) and divided once, as avg_pool2d does.
template <bool UNIFORM>
__global__ void __launch_bounds__(256) image_metrics_kernel(const float* x, const float* ref, float* out, int C, int H, int W, float data_range,
                                                            Taps taps, int win, double cov_norm, double k1, double k2) {
  __shared__ double sh_se[4], sh_ss[4];
  __shared__ float sh_mn[4], sh_mx[4];
  __shared__ double tp[MAX_WIN];
  __shared__ float sx[IR_MAX * IC_MAX], sy[IR_MAX * IC_MAX];
  __shared__ double hs[5][IR_MAX * TW];
  const int tid = threadIdx.x;
  const int64_t plane = (int64_t)H * W, per = plane * C;
  const float* xs = x + (int64_t)blockIdx.x * per;
  const float* ys = ref + (int64_t)blockIdx.x * per;
  if (tid < MAX_WIN) tp[tid] = tid < win ? (double)taps.t[tid] : 0.0;

  // ---- phase 1: squared error (the loop, the shuffles and the four-entry combine of mse_per_sample_kernel: same bits), min and max of ref
  double se = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int64_t i = tid; i < per; i += 256) {
    const float r = ys[i], d = xs[i] - r;
    se += (double)d * (double)d;
    mn = fminf(mn, r); mx = fmaxf(mx, r);
  }
  for (int o = 32; o > 0; o >>= 1) {
    se += __shfl_xor(se, o);
    mn = fminf(mn, __shfl_xor(mn, o)); mx = fmaxf(mx, __shfl_xor(mx, o));
  }
  if ((tid & 63) == 0) { sh_se[tid >> 6] = se; sh_mn[tid >> 6] = mn; sh_mx[tid >> 6] = mx; }
  __syncthreads();
  const double mse = (sh_se[0] + sh_se[1] + sh_se[2] + sh_se[3]) / (double)per;
  const double R = data_range > 0.f ? (double)data_range
                                    : (double)fmaxf(fmaxf(sh_mx[0], sh_mx[1]), fmaxf(sh_mx[2], sh_mx[3])) -
                                          (double)fminf(fminf(sh_mn[0], sh_mn[1]), fminf(sh_mn[2], sh_mn[3]));
  const double C1 = (k1 * R) * (k1 * R), C2 = (k2 * R) * (k2 * R);

  // ---- phase 2: SSIM over the OH x OW window positions of every channel
  const int OH = H - win + 1, OW = W - win + 1;
  const double area = (double)(win * win);
  double acc = 0.0;
  for (int c = 0; c < C; ++c) {
    const float* px = xs + (int64_t)c * plane;
    const float* py = ys + (int64_t)c * plane;
    for (int r0 = 0; r0 < OH; r0 += TH) {
      const int th = min(TH, OH - r0), ir = th + win - 1;
      for (int c0 = 0; c0 < OW; c0 += TW) {
        const int tw = min(TW, OW - c0), ic = tw + win - 1;
        // stage the patch (its last readers, the previous tile's horizontal pass, are behind that tile's second barrier)
        for (int i = tid; i < ir * ic; i += 256) {
          const int r = i / ic, cc = i - r * ic;
          const int64_t g = (int64_t)(r0 + r) * W + (c0 + cc);
          sx[r * IC_MAX + cc] = px[g];
          sy[r * IC_MAX + cc] = py[g];
        }
        __syncthreads();   // also: the previous tile's vertical pass has finished reading hs
        // horizontal window sums of x, y, xx, yy, xy for every patch row
        for (int i = tid; i < ir * TW; i += 256) {
          const int r = i / TW, cc = i % TW;
          if (cc < tw) {
            double a = 0.0, b = 0.0, aa = 0.0, bb = 0.0, ab = 0.0;
            for (int k = 0; k < win; ++k) {
              const double u = (double)sx[r * IC_MAX + cc + k], v = (double)sy[r * IC_MAX + cc + k];
              if (UNIFORM) { a += u; b += v; aa += u * u; bb += v * v; ab += u * v; }
              else { const double t = tp[k]; a += t * u; b += t * v; aa += t * (u * u); bb += t * (v * v); ab += t * (u * v); }
            }
            hs[0][i] = a; hs[1][i] = b; hs[2][i] = aa; hs[3][i] = bb; hs[4][i] = ab;
          }
        }
        __syncthreads();
        // vertical sums, S, per-thread accumulation in a fixed order
        for (int i = tid; i < th * TW; i += 256) {
          const int cc = i % TW;
          if (cc < tw) {
            double ux = 0.0, uy = 0.0, uxx = 0.0, uyy = 0.0, uxy = 0.0;
            for (int k = 0; k < win; ++k) {
              const int j = i + k * TW;
              if (UNIFORM) { ux += hs[0][j]; uy += hs[1][j]; uxx += hs[2][j]; uyy += hs[3][j]; uxy += hs[4][j]; }
              else { const double t = tp[k]; ux += t * hs[0][j]; uy += t * hs[1][j]; uxx += t * hs[2][j]; uyy += t * hs[3][j]; uxy += t * hs[4][j]; }
            }
            if (UNIFORM) { ux /= area; uy /= area; uxx /= area; uyy /= area; uxy /= area; }
            const double vx = cov_norm * (uxx - ux * ux), vy = cov_norm * (uyy - uy * uy), vxy = cov_norm * (uxy - ux * uy);
            acc += ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2));
          }
        }
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if ((tid & 63) == 0) sh_ss[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float* o = out + (int64_t)blockIdx.x * 4;
    o[0] = (float)mse;
    o[1] = (float)R;
    o[2] = (float)(10.0 * log10((R * R) / mse));   // IEEE: +inf for identical images, -inf for R = 0, NaN for 0 / 0
    o[3] = (float)((sh_ss[0] + sh_ss[1] + sh_ss[2] + sh_ss[3]) / ((double)C * (double)OH * (double)OW));
  }
}

}  // namespace

int image_metrics_launch(const float* x, const float* ref, float* out, int batch, int channels, int h, int w, float data_range,
                         const float* taps_host, int win, float cov_norm, float k1, float k2, hipStream_t s) {
  MI355_REQUIRE(batch >= 1, -1, "image_metrics: batch must be at least 1");
  MI355_REQUIRE(channels >= 1, -1, "image_metrics: channels must be at least 1");
  MI355_REQUIRE(h >= 1 && h <= 4096, -1, "image_metrics: h must be in 1..4096");
  MI355_REQUIRE(w >= 1 && w <= 4096, -1, "image_metrics: w must be in 1..4096");
  MI355_REQUIRE((win & 1) == 1 && win >= 3 && win <= MAX_WIN, -1, "image_metrics: win must be odd and in 3..15");
  MI355_REQUIRE(win <= h && win <= w, -1, "image_metrics: win must not exceed min(h, w)");
  MI355_REQUIRE(k1 >= 0.f, -1, "image_metrics: k1 must not be negative");
  MI355_REQUIRE(k2 >= 0.f, -1, "image_metrics: k2 must not be negative");
  MI355_REQUIRE(cov_norm > 0.f, -1, "image_metrics: cov_norm must be positive");
  Taps taps;
  for (int k = 0; k < MAX_WIN; ++k) taps.t[k] = (taps_host && k < win) ? taps_host[k] : 0.f;
  if (taps_host)
    hipLaunchKernelGGL(image_metrics_kernel<false>, dim3((unsigned)batch), dim3(256), 0, s, x, ref, out, channels, h, w, data_range, taps, win,
                       (double)cov_norm, (double)k1, (double)k2);
  else
    hipLaunchKernelGGL(image_metrics_kernel<true>, dim3((unsigned)batch), dim3(256), 0, s, x, ref, out, channels, h, w, data_range, taps, win,
                       (double)cov_norm, (double)k1, (double)k2);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
