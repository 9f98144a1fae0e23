// Tiled sampling (MultiDiffusion, Bar-Tal et al. 2023): a canvas [B, C, Hc, Wc] larger than the net's S x S frame is cut into overlapping S x S
// windows, the net runs on the windows as one batch, and the predictions are fused per pixel by a weighted average.  Two HBM-bound kernels per
// evaluation over fp32 NCHW tensors, and the geometry both of them, the C ABI and the Python binding share.
//
// Geometry: along an axis of length L >= S with stride 1 <= s <= S there are n = ceil((L - S) / s) + 1 windows at o_i = min(i * s, L - S): the last
// one is clamped to the edge, so every pixel is covered and no window leaves the canvas.  Window w = iy * nx + ix of canvas b is batch row b * nW + w.
// Weights are separable, p(dy) * p(dx) over the offsets inside the window: uniform p = 1, tent p(i) = min(i + 1, S - i) (small integers, exact in
// fp32, positive everywhere).  They are generated from the offsets: there is no weight tensor.
//
// tile_blend's order is its contract: for each canvas element, over the windows that cover it in ASCENDING window index, num += weight * v (product,
// then sum, each rounded) and den += weight; then vbar = num / den (correctly rounded), and with euler_x: x <- x + dt * vbar (product, sum).  It is a
// gather on the canvas side (one thread per canvas element group, no atomics), bit-exact against the eager fp32 expression in that order.
#include <string>

#include "ops.h"

#pragma clang fp contract(off)

int tile_geom(int image_size, const mi355_tile_plan* plan, TileGeom* g, const char* who) {
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(plan && g, -1, f + "plan is null");
  MI355_REQUIRE(image_size >= 1, -1, f + "image_size must be >= 1");
  const int S = image_size;
  MI355_REQUIRE(plan->canvas_h >= S, -2, f + "canvas_h is smaller than the net's image_size");
  MI355_REQUIRE(plan->canvas_w >= S, -2, f + "canvas_w is smaller than the net's image_size");
  MI355_REQUIRE(plan->stride_y >= 1 && plan->stride_y <= S, -1, f + "stride_y must be in 1..image_size");
  MI355_REQUIRE(plan->stride_x >= 1 && plan->stride_x <= S, -1, f + "stride_x must be in 1..image_size");
  MI355_REQUIRE(plan->weight == MI355_TILE_UNIFORM || plan->weight == MI355_TILE_TENT, -1, f + "weight must be MI355_TILE_UNIFORM or MI355_TILE_TENT");
  MI355_REQUIRE(plan->chunk >= 1, -1, f + "chunk must be >= 1");
  g->S = S; g->Hc = plan->canvas_h; g->Wc = plan->canvas_w; g->sy = plan->stride_y; g->sx = plan->stride_x; g->weight = plan->weight;
  g->ny = (g->Hc - S + g->sy - 1) / g->sy + 1;
  g->nx = (g->Wc - S + g->sx - 1) / g->sx + 1;
  const int64_t nW = (int64_t)g->ny * g->nx;
  MI355_REQUIRE(nW < (1 << 24), -4, f + "canvas_h / canvas_w: more than 2^24 windows per canvas");
  g->nW = (int)nW;
  return 0;
}

namespace {

__device__ inline int origin(int i, int s, int L, int S) { const int o = i * s; return o < L - S ? o : L - S; }
// the windows i_lo..i_hi along one axis that cover position p (every i between them does: only the last origin is clamped, towards smaller values)
__device__ inline void cover(int p, int s, int L, int S, int n, int& lo, int& hi) {
  lo = p >= S ? (p - S) / s + 1 : 0;
  hi = p >= L - S ? n - 1 : p / s;
}
__device__ inline float taper(int weight, int d, int S) { return weight == MI355_TILE_TENT ? (float)(d + 1 < S - d ? d + 1 : S - d) : 1.f; }

// windows[(b * nW + w), c, dy, dx] = canvas[b, c, oy + dy, ox + dx]; one thread per four consecutive window elements.  VEC: S % 4 == 0, so the four
// share a window row; they leave as one 16-byte store and arrive as one 16-byte load where the canvas address allows it.
template <bool VEC>
__global__ void __launch_bounds__(256) tile_gather_kernel(const float* __restrict__ canvas, float* __restrict__ win, int64_t n, int C, TileGeom g) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  const int S = g.S;
  auto src = [&](int64_t e) -> int64_t {
    const int dx = (int)(e % S); int64_t r = e / S;
    const int dy = (int)(r % S); r /= S;
    const int c = (int)(r % C); r /= C;
    const int w = (int)(r % g.nW); const int64_t b = r / g.nW;
    const int oy = origin(w / g.nx, g.sy, g.Hc, S), ox = origin(w % g.nx, g.sx, g.Wc, S);
    return ((b * C + c) * g.Hc + (oy + dy)) * (int64_t)g.Wc + (ox + dx);
  };
  if (VEC) {
    const int64_t sidx = src(i);
    const float* p = canvas + sidx;
    f32x4 v;
    if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) v = *reinterpret_cast<const f32x4*>(p);
    else v = f32x4{p[0], p[1], p[2], p[3]};
    *reinterpret_cast<f32x4*>(win + i) = v;
  } else {
    const int cnt = n - i < 4 ? (int)(n - i) : 4;
    for (int j = 0; j < cnt; ++j) win[i + j] = canvas[src(i + j)];
  }
}

__global__ void __launch_bounds__(256) tile_labels_kernel(const int32_t* __restrict__ labels, int32_t* __restrict__ out, int64_t n, int nW) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = labels[i / nW];
}

// One thread per G consecutive canvas elements of a row (G = 4 where Wc % 4 == 0, else 1).  For every window row iy and column ix that can cover one
// of them, in ascending w = iy * nx + ix, each covered element takes num += weight * v, den += weight.
template <int G>
__global__ void __launch_bounds__(256) tile_blend_kernel(const float* __restrict__ win, float* __restrict__ vbar, float* __restrict__ euler_x, float dt,
                                                         int64_t n, int C, TileGeom g) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * G;
  if (i >= n) return;
  const int S = g.S;
  const int x0 = (int)(i % g.Wc); int64_t r = i / g.Wc;
  const int y = (int)(r % g.Hc); r /= g.Hc;
  const int c = (int)(r % C); const int64_t b = r / C;
  int iy_lo, iy_hi, ix_lo, ix_hi, t0, t1;
  cover(y, g.sy, g.Hc, S, g.ny, iy_lo, iy_hi);
  cover(x0, g.sx, g.Wc, S, g.nx, ix_lo, t1);
  cover(x0 + G - 1, g.sx, g.Wc, S, g.nx, t0, ix_hi);
  float num[G], den[G];
#pragma unroll
  for (int j = 0; j < G; ++j) { num[j] = 0.f; den[j] = 0.f; }
  for (int iy = iy_lo; iy <= iy_hi; ++iy) {
    const int dy = y - origin(iy, g.sy, g.Hc, S);
    if (dy < 0 || dy >= S) continue;
    const float py = taper(g.weight, dy, S);
    for (int ix = ix_lo; ix <= ix_hi; ++ix) {
      const int dx0 = x0 - origin(ix, g.sx, g.Wc, S);
      const float* row = win + ((((b * g.nW + (int64_t)iy * g.nx + ix) * C + c) * S + dy) * (int64_t)S);
      float v[G];
      bool in[G];
#pragma unroll
      for (int j = 0; j < G; ++j) in[j] = dx0 + j >= 0 && dx0 + j < S;
      if (G == 4 && dx0 >= 0 && dx0 + 3 < S && (reinterpret_cast<uintptr_t>(row + dx0) & 15) == 0) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(row + dx0);
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = t[j];
      } else {
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = in[j] ? row[dx0 + j] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < G; ++j) {
        if (!in[j]) continue;
        const float wgt = py * taper(g.weight, dx0 + j, S);   // small integers: exact
        const float p = wgt * v[j];
        num[j] = num[j] + p;
        den[j] = den[j] + wgt;
      }
    }
  }
  float o[G];
#pragma unroll
  for (int j = 0; j < G; ++j) o[j] = num[j] / den[j];
  const bool al = G == 4 && (reinterpret_cast<uintptr_t>(vbar + i) & 15) == 0 && (!euler_x || (reinterpret_cast<uintptr_t>(euler_x + i) & 15) == 0);
  if (al) {
    *reinterpret_cast<f32x4*>(vbar + i) = f32x4{o[0], o[1], o[2], o[3]};
    if (euler_x) {
      f32x4 xv = *reinterpret_cast<const f32x4*>(euler_x + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) { const float p = dt * o[j]; xv[j] = xv[j] + p; }
      *reinterpret_cast<f32x4*>(euler_x + i) = xv;
    }
  } else {
#pragma unroll
    for (int j = 0; j < G; ++j) {
      vbar[i + j] = o[j];
      if (euler_x) { const float p = dt * o[j]; euler_x[i + j] = euler_x[i + j] + p; }
    }
  }
}

inline int check_count(const char* who, int64_t n) {
  MI355_REQUIRE(n / 4 / 256 < 0x7FFFFFFFll, -4, std::string(who) + ": too many elements for one launch");
  return 0;
}

}  // namespace

int tile_gather_launch(const float* canvas, float* windows, int B, int C, const TileGeom& g, hipStream_t s) {
  MI355_REQUIRE(canvas && windows && B > 0 && C > 0, -1, "tile_gather: bad argument");
  const int64_t n = (int64_t)B * g.nW * C * g.S * g.S;
  if (int rc = check_count("tile_gather", n)) return rc;
  const unsigned blocks = (unsigned)(((n + 3) / 4 + 255) / 256);
  if (g.S % 4 == 0 && (reinterpret_cast<uintptr_t>(windows) & 15) == 0)
    hipLaunchKernelGGL(tile_gather_kernel<true>, dim3(blocks), dim3(256), 0, s, canvas, windows, n, C, g);
  else
    hipLaunchKernelGGL(tile_gather_kernel<false>, dim3(blocks), dim3(256), 0, s, canvas, windows, n, C, g);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int tile_labels_launch(const int32_t* labels, int32_t* out, int B, int nW, hipStream_t s) {
  MI355_REQUIRE(labels && out && B > 0 && nW > 0, -1, "tile_labels: bad argument");
  const int64_t n = (int64_t)B * nW;
  hipLaunchKernelGGL(tile_labels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, labels, out, n, nW);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int tile_blend_launch(const float* windows, float* vbar, float* euler_x, float dt, int B, int C, const TileGeom& g, hipStream_t s) {
  MI355_REQUIRE(windows && vbar && B > 0 && C > 0, -1, "tile_blend: bad argument");
  MI355_REQUIRE(vbar != euler_x, -1, "tile_blend: vbar and euler_x must be different buffers");
  const int64_t n = (int64_t)B * C * g.Hc * g.Wc;
  if (int rc = check_count("tile_blend", n)) return rc;
  if (g.Wc % 4 == 0)
    hipLaunchKernelGGL(tile_blend_kernel<4>, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, windows, vbar, euler_x, dt, n, C, g);
  else
    hipLaunchKernelGGL(tile_blend_kernel<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, windows, vbar, euler_x, dt, n, C, g);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
