// The null-space (DDNM) predictor step: Wang, Yu, Zhang, "Zero-Shot Image Restoration Using Denoising Diffusion Null-Space Model", ICLR 2023.  The
// data prediction of a DDPM step is rectified against a linear measurement y = A x before the step moves the state from it,
//   x0  = clip_nan(x0_pre(kind of prediction), -1, 1)          the data prediction of every step in steps.hip (Pred<K>, step_common.h)
//   r_q = A(x0)_q - y_q                                        the residual of measurement row q
//   x0h = x0 - lam * r_q(p)  where p is a tap of row q, else x0
//   form 0: x <- (coef1 * x0h + coef2 * x) + sigma * z         the ancestral step
//   form 1: x <- sa * x0h + sb * e2 (+ sigma * z),  e2 = (c_recip * x - x0h) / c_recipm1      the DDIM(eta) step of steps.hip on x0h
// every operation rounded to fp32, none contracted.  The operators (mi355_nullspace_op) are row operators with disjoint supports and equal weights
// inside a row, so A A^T is diagonal and the pseudo-inverse A^+ r puts r_q itself on every tap of q:
//   kind 0  mask         a pixel is a row iff y != pad_value; element-wise, on the flat launch of steps.hip
//   kind 1  block mean   row q = the sy x sx block of q, weights 1 / (sy sx): A(x0)_q = S_q / (float)(sy sx), one division
//   kind 2  bilinear     row q = the taps of mi355_resize_bilinear for an integer factor: along an axis an even factor s has the two taps
//                        s o + s / 2 - 1 and s o + s / 2 (weights 1/2, 1/2), an odd one the single tap s o + (s - 1) / 2 (weight 1);
//                        A(x0)_q = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11), the kernel's operation order; a tap of weight 0 is not
//                        read and enters as 0.f, which gives the resize kernel's bits on finite data and keeps a NaN outside the taps to itself
//
// Kinds 1 and 2 are ONE launch that is not element-wise.  The state [planes, H, W] is a matrix of planes * H rows of W floats in which a band (the sy
// rows of one row of blocks) is contiguous and bands follow each other across planes; a workgroup of 256 threads owns a tile of whole bands: `bands`
// consecutive bands over the whole width where they are small (planes mix freely, the last tile may be short), or one band cut into column chunks of
// whole blocks where a band is wider than a workgroup's 1024 quads.  It reads x, the network output (under its image stride) once, 16 bytes per lane
// where the address allows (ld4 / st4: any W, any pointer offset), keeps x and x0 in registers and x0 in LDS, reduces in LDS, reads y once per block,
// and writes x once.  Nothing goes through global memory in between and there are no atomics.
//
// The summation order of S_q (kind 1) is fixed: each of the block's sy rows left to right (sx - 1 sums), then the sy row sums top to bottom (sy - 1
// sums).  block_mean_launch runs the same two loops on the same tiling, so mi355_block_mean(x0) is A(x0) of the step bit for bit, and two runs agree.
#include <cmath>
#include <string>

#include "ops.h"

#pragma clang fp contract(off)

#include "step_common.h"

namespace {

constexpr int NS_THREADS = 256, NS_QPT = 4, NS_MAXQ = NS_THREADS * NS_QPT;   // quads (four columns of a row) per thread and per tile
constexpr int NS_TILE = 4 * NS_MAXQ;                                          // floats of a tile at the most

// The tiling of a [rows = planes * H][W] matrix with sy x sx blocks: tiles of bands * sy rows and gpc * sx columns (the last of either may be short).
struct NsTiling {
  int W, sy, sx, w_low, gpc, n_chunks, bands;
  int64_t total_bands, n_rowblocks;
};
NsTiling ns_tiling(int64_t planes, int H, int W, int sy, int sx) {
  NsTiling t = {};
  t.W = W; t.sy = sy; t.sx = sx; t.w_low = W / sx;
  t.total_bands = planes * (H / sy);
  const int max_cols = 4 * (NS_MAXQ / sy);            // >= 128 >= sx: one column of blocks always fits
  t.gpc = t.w_low < max_cols / sx ? t.w_low : max_cols / sx;
  t.n_chunks = (t.w_low + t.gpc - 1) / t.gpc;
  t.bands = 1;
  if (t.gpc == t.w_low) {   // a band fits: several per workgroup, at least a workgroup's worth of quads, more only while a thousand workgroups remain
    const int qpb = sy * ((W + 3) / 4);
    const int64_t hi = NS_MAXQ / qpb;
    int64_t lo = (NS_THREADS + qpb - 1) / qpb;
    if (lo > hi) lo = hi;
    int64_t b = t.total_bands / 1024;
    b = b < lo ? lo : (b > hi ? hi : b);
    if (b > t.total_bands) b = t.total_bands;
    t.bands = (int)(b < 1 ? 1 : b);
  }
  t.n_rowblocks = (t.total_bands + t.bands - 1) / t.bands;
  return t;
}

// What a thread knows of its tile (every quantity uniform over the workgroup)
struct NsTile {
  int64_t row0;        // first row of the tile in the [planes * H][W] matrix
  int rows, col0, cw;  // its rows (whole bands), first column, columns (whole blocks)
  int gh, qpr;         // blocks per band row, quads per row
};
__device__ inline NsTile ns_tile(const NsTiling& t) {
  NsTile k;
  const int64_t rb = blockIdx.x / t.n_chunks;
  const int ch = (int)(blockIdx.x - rb * t.n_chunks);
  const int64_t band0 = rb * t.bands;
  const int64_t nb = t.total_bands - band0 < t.bands ? t.total_bands - band0 : t.bands;
  k.row0 = band0 * t.sy; k.rows = (int)nb * t.sy;
  const int g0 = ch * t.gpc;
  k.gh = t.w_low - g0 < t.gpc ? t.w_low - g0 : t.gpc;
  k.col0 = g0 * t.sx; k.cw = k.gh * t.sx;
  k.qpr = (k.cw + 3) / 4;
  return k;
}

// S_q / (sy sx) of every block of the tile from its values in LDS (v: [rows][cw]), in the order of the file comment; f(band of the tile, block of the
// band, mean).  rs: [rows][gh] scratch.  Ends behind a barrier only where the caller adds one.
template <typename F>
__device__ inline void ns_block_means(const NsTiling& t, const NsTile& k, const float* v, float* rs, F f) {
  const int tid = threadIdx.x;
  for (int it = tid; it < k.rows * k.gh; it += NS_THREADS) {
    const int r = it / k.gh, g = it - r * k.gh;
    const float* p = v + r * k.cw + g * t.sx;
    float s = p[0];
    for (int j = 1; j < t.sx; ++j) s = s + p[j];
    rs[it] = s;
  }
  __syncthreads();
  const float cnt = (float)(t.sy * t.sx);
  for (int it = tid; it < k.rows / t.sy * k.gh; it += NS_THREADS) {
    const int b = it / k.gh, g = it - b * k.gh;
    const float* p = rs + b * t.sy * k.gh + g;
    float s = p[0];
    for (int j = 1; j < t.sy; ++j) s = s + p[j * k.gh];
    f(b, g, s / cnt);
  }
}

__global__ void __launch_bounds__(NS_THREADS) block_mean_kernel(NsTiling t, const float* __restrict__ in, float* __restrict__ out) {
  __shared__ float v[NS_TILE], rs[NS_TILE];
  const NsTile k = ns_tile(t);
  const int tid = threadIdx.x;
  for (int q = tid; q < k.rows * k.qpr; q += NS_THREADS) {
    const int r = q / k.qpr, c = (q - r * k.qpr) * 4;
    const int cnt = k.cw - c < 4 ? k.cw - c : 4;
    float a[4];
    ld4(in, (k.row0 + r) * t.W + k.col0 + c, cnt, a);
    for (int l = 0; l < cnt; ++l) v[r * k.cw + c + l] = a[l];
  }
  __syncthreads();
  const int64_t q0 = k.row0 / t.sy * t.w_low + k.col0 / t.sx;
  ns_block_means(t, k, v, rs, [&](int b, int g, float m) { out[q0 + (int64_t)b * t.w_low + g] = m; });
}

struct NsArgs {
  float* x; const float* out; const float* y; const float* z;
  int64_t per, stride, rows_per_image;   // elements and rows of an image of the state; the image stride of `out`
  float c_recip, c_recipm1, a, b, sigma, lam;
  int noisy, use_philox; uint64_t seed, off4;
};
// the move of one element from its rectified data prediction
template <int FORM>
__device__ inline float ns_move(const NsArgs& a, float x, float x0h, float z) {
  if constexpr (FORM == 0) {
    const float mean = a.a * x0h + a.b * x;
    return mean + a.sigma * z;
  } else {
    const float e2 = (a.c_recip * x - x0h) / a.c_recipm1;   // the eps the RECTIFIED prediction stands for
    const float m = a.a * x0h + a.b * e2;
    return a.noisy ? m + a.sigma * z : m;
  }
}
// the draw of elements i .. i + cnt - 1 of the state: injected, or Philox element by element (a quad of a row need not sit on the stream's groups of four)
__device__ inline void ns_noise(const NsArgs& a, int64_t i, int cnt, float (&zz)[4]) {
  zz[0] = zz[1] = zz[2] = zz[3] = 0.f;
  if (a.z) { ld4(a.z, i, cnt, zz); return; }
  if (!a.use_philox) return;
  if ((i & 3) == 0) { randn4(a.seed, a.off4 + (uint64_t)(i >> 2), zz); return; }
  float g[4];
  int64_t cur = -1;
  for (int l = 0; l < cnt; ++l) {
    const int64_t e = i + l;
    if ((e >> 2) != cur) { cur = e >> 2; randn4(a.seed, a.off4 + (uint64_t)cur, g); }
    zz[l] = g[e & 3];
  }
}

// the taps of a block along an axis of factor s (file comment): first tap, and whether there is a second one behind it
__device__ inline int ns_tap0(int s) { return (s & 1) ? (s - 1) / 2 : s / 2 - 1; }

template <int KIND, int FORM, class P>
__global__ void __launch_bounds__(NS_THREADS) nullspace_step_kernel(NsTiling t, NsArgs a, P pr) {
  __shared__ float v[NS_TILE], rs[NS_TILE], res[NS_TILE];
  const NsTile k = ns_tile(t);
  const int tid = threadIdx.x, nq = k.rows * k.qpr;
  float xv[NS_QPT][4], x0v[NS_QPT][4];
#pragma unroll
  for (int u = 0; u < NS_QPT; ++u) {
    const int q = tid + u * NS_THREADS;
    if (q >= nq) continue;
    const int r = q / k.qpr, c = (q - r * k.qpr) * 4;
    const int cnt = k.cw - c < 4 ? k.cw - c : 4;
    const int64_t row = k.row0 + r, i = row * t.W + k.col0 + c;
    const int64_t img = row / a.rows_per_image;
    float ov[4];
    ld4(a.x, i, cnt, xv[u]);
    ld4(a.out + img * a.stride + (i - img * a.per), 0, cnt, ov);
#pragma unroll
    for (int l = 0; l < 4; ++l) x0v[u][l] = clip_nan(pr.pre(a.c_recip, a.c_recipm1, xv[u][l], ov[l]), -1.f, 1.f);
    for (int l = 0; l < cnt; ++l) v[r * k.cw + c + l] = x0v[u][l];
  }
  __syncthreads();
  const int64_t q0 = k.row0 / t.sy * t.w_low + k.col0 / t.sx;
  if constexpr (KIND == 1) {
    ns_block_means(t, k, v, rs, [&](int b, int g, float m) { res[b * k.gh + g] = m - a.y[q0 + (int64_t)b * t.w_low + g]; });
  } else {
    const int ty = ns_tap0(t.sy), tx = ns_tap0(t.sx);
    const float l1y = (t.sy & 1) ? 0.f : 0.5f, l1x = (t.sx & 1) ? 0.f : 0.5f;
    const float l0y = 1.f - l1y, l0x = 1.f - l1x;
    for (int it = tid; it < k.rows / t.sy * k.gh; it += NS_THREADS) {
      const int b = it / k.gh, g = it - b * k.gh;
      const float* p = v + (b * t.sy + ty) * k.cw + g * t.sx + tx;
      const float v00 = p[0], v01 = l1x != 0.f ? p[1] : 0.f;
      const float v10 = l1y != 0.f ? p[k.cw] : 0.f, v11 = (l1y != 0.f && l1x != 0.f) ? p[k.cw + 1] : 0.f;
      const float d = l0y * (l0x * v00 + l1x * v01) + l1y * (l0x * v10 + l1x * v11);
      res[it] = d - a.y[q0 + (int64_t)b * t.w_low + g];
    }
  }
  __syncthreads();
  const int ty = ns_tap0(t.sy), tx = ns_tap0(t.sx);
  const int ty1 = (t.sy & 1) ? ty : ty + 1, tx1 = (t.sx & 1) ? tx : tx + 1;
#pragma unroll
  for (int u = 0; u < NS_QPT; ++u) {
    const int q = tid + u * NS_THREADS;
    if (q >= nq) continue;
    const int r = q / k.qpr, c = (q - r * k.qpr) * 4;
    const int cnt = k.cw - c < 4 ? k.cw - c : 4;
    const int64_t i = (k.row0 + r) * t.W + k.col0 + c;
    const int b = r / t.sy, ry = r - b * t.sy;
    float zz[4], o[4];
    ns_noise(a, i, cnt, zz);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const int col = c + l < k.cw ? c + l : k.cw - 1;   // lanes behind the row's end are computed and not stored
      const int g = col / t.sx, rx = col - g * t.sx;
      const bool tap = KIND == 1 || ((ry == ty || ry == ty1) && (rx == tx || rx == tx1));
      const float d = a.lam * res[b * k.gh + g];
      const float x0h = tap ? x0v[u][l] - d : x0v[u][l];
      o[l] = ns_move<FORM>(a, xv[u][l], x0h, zz[l]);
    }
    st4(a.x, i, cnt, o);
  }
}

template <int FORM, class P>
int nullspace_mask_form(const NsArgs& a, P pr, float pad, int64_t n, hipStream_t s) {
  return launch_ew4(n, s, [=] __device__(int64_t i, int64_t i4, int cnt) {
    float xv[4], ov[4], yv[4], zz[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    ld4(a.x, i, cnt, xv);
    ld4_eps(a.out, a.per, a.stride, i, cnt, ov);
    ld4(a.y, i, cnt, yv);
    if (FORM == 0 || a.noisy) noise4(a.z, a.use_philox, a.seed, a.off4, i, i4, cnt, zz);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x0 = clip_nan(pr.pre(a.c_recip, a.c_recipm1, xv[j], ov[j]), -1.f, 1.f);
      const float r = x0 - yv[j];
      const float d = a.lam * r;
      const float x0h = yv[j] == pad ? x0 : x0 - d;   // y == pad_value: unknown, pure null space
      o[j] = ns_move<FORM>(a, xv[j], x0h, zz[j]);
    }
    st4(a.x, i, cnt, o);
  });
}

template <int KIND, int FORM, class P>
int nullspace_band_form(const NsTiling& t, const NsArgs& a, P pr, hipStream_t s) {
  hipLaunchKernelGGL((nullspace_step_kernel<KIND, FORM, P>), dim3((unsigned)(t.n_rowblocks * t.n_chunks)), dim3(NS_THREADS), 0, s, t, a, pr);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

}  // namespace

// Every refusal of a mi355_nullspace_op against a state of h x w pixels, before any launch, each naming its argument (h, w > 0: the caller's check).
int check_nullspace_op(const char* who, const mi355_nullspace_op* op, int h, int w) {
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(op, -1, f + "op is null");
  MI355_REQUIRE(op->kind >= 0 && op->kind <= 2, -1, f + "op->kind must be 0 (mask), 1 (block mean) or 2 (bilinear taps)");
  if (op->kind == 0) return 0;
  MI355_REQUIRE(op->h_low >= 1 && op->w_low >= 1, -1, f + "op->h_low and op->w_low must be >= 1");
  MI355_REQUIRE(h % op->h_low == 0 && w % op->w_low == 0, -4,
                f + "op->h_low, op->w_low must divide the state's height and width (integer factors only: the rows of A are then disjoint)");
  MI355_REQUIRE(h / op->h_low <= 32 && w / op->w_low <= 32, -4, f + "op->h_low, op->w_low: factors 1..32 per axis are built");
  return 0;
}

int nullspace_step_launch(const NullspaceStep& p, hipStream_t s) {
  const char* const who = "nullspace_step";
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(p.form == 0 || p.form == 1, -1, f + "form must be 0 (ancestral) or 1 (DDIM(eta))");
  MI355_REQUIRE(p.pred >= PRED_EPS && p.pred <= PRED_V, -1, f + "pred_kind must be 0 (eps), 1 (x0) or 2 (v)");
  MI355_REQUIRE(p.batch >= 0 && p.channels > 0 && p.h > 0 && p.w > 0, -1, f + "batch must be >= 0 and channels, h, w > 0");
  if (int rc = check_nullspace_op(who, p.op, p.h, p.w)) return rc;
  MI355_REQUIRE(p.lam >= 0.f && p.lam <= 1.f, -1, f + "lam must be in [0, 1]");
  MI355_REQUIRE(p.sigma >= 0.f && p.sigma <= 3.0e38f, -1, f + "sigma must be finite and >= 0");
  MI355_REQUIRE(p.offset % 4 == 0, -1, f + "the Philox offset must be a multiple of 4");
  const int64_t per = (int64_t)p.channels * p.h * p.w, n = (int64_t)p.batch * per;
  const int64_t stride = p.out_stride ? p.out_stride : per;
  MI355_REQUIRE(stride >= per, -1, f + "out_stride must be 0 (contiguous) or >= channels * h * w");
  if (n <= 0) return 0;
  MI355_REQUIRE(p.x && p.out && p.y, -1, f + "null argument (x, out, y)");
  NsArgs a = {};
  a.x = p.x; a.out = p.out; a.y = p.y; a.z = p.z;
  a.per = per; a.stride = stride; a.rows_per_image = (int64_t)p.channels * p.h;
  a.c_recip = p.c_recip; a.c_recipm1 = p.c_recipm1; a.sigma = p.sigma; a.lam = p.lam;
  a.use_philox = p.use_philox; a.seed = p.seed; a.off4 = p.offset / 4;
  a.noisy = p.z != nullptr || p.use_philox;
  if (p.form == 0) { a.a = p.a; a.b = p.b; }
  else { const DdimEta c = ddim_eta_coefs(p.a, p.sigma); a.a = c.sa; a.b = c.sb; }
  const int kind = p.op->kind, form = p.form;
  if (kind == 0) {
    const float pad = p.op->pad_value;
    return pred_form(p.pred, p.sa, p.sb, [&](auto pr) {
      return form == 0 ? nullspace_mask_form<0>(a, pr, pad, n, s) : nullspace_mask_form<1>(a, pr, pad, n, s);
    });
  }
  const NsTiling t = ns_tiling((int64_t)p.batch * p.channels, p.h, p.w, p.h / p.op->h_low, p.w / p.op->w_low);
  MI355_REQUIRE(t.n_rowblocks * t.n_chunks < ((int64_t)1 << 31), -2, f + "the state has more tiles than a launch has workgroups");
  return pred_form(p.pred, p.sa, p.sb, [&](auto pr) {
    if (kind == 1) return form == 0 ? nullspace_band_form<1, 0>(t, a, pr, s) : nullspace_band_form<1, 1>(t, a, pr, s);
    return form == 0 ? nullspace_band_form<2, 0>(t, a, pr, s) : nullspace_band_form<2, 1>(t, a, pr, s);
  });
}

int block_mean_launch(const float* in, float* out, int64_t planes, int h, int w, int h_low, int w_low, hipStream_t s) {
  const std::string f = "block_mean: ";
  MI355_REQUIRE(planes >= 0 && h > 0 && w > 0, -1, f + "planes must be >= 0 and h, w > 0");
  mi355_nullspace_op op = {};
  op.kind = 1; op.h_low = h_low; op.w_low = w_low;
  if (int rc = check_nullspace_op("block_mean", &op, h, w)) return rc;
  if (planes == 0) return 0;
  MI355_REQUIRE(in && out, -1, f + "null argument (in, out)");
  MI355_REQUIRE(in != out, -1, f + "out must not be in");
  const NsTiling t = ns_tiling(planes, h, w, h / h_low, w / w_low);
  MI355_REQUIRE(t.n_rowblocks * t.n_chunks < ((int64_t)1 << 31), -2, f + "the input has more tiles than a launch has workgroups");
  hipLaunchKernelGGL(block_mean_kernel, dim3((unsigned)(t.n_rowblocks * t.n_chunks)), dim3(NS_THREADS), 0, s, t, in, out);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
