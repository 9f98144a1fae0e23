// Sinusoidal timestep embedding + the small fp32 linears around it, and NCHW<->NHWC boundary packing.
//
// Reference: timestep_embedding (AD/image_diffusion/nn.py:97-115), UNetModel.time_embed
// (unet.py:564-569: Linear, SiLU, Linear) and every ResBlock's emb_layers (unet.py:297-305: SiLU,
// Linear) - the latter are batched into ONE linear over the concatenated output channels of all
// ResBlocks per forward.  All fp32 (the reference forces fp32 here, nn.py:111).
// Class-conditional nets add label_emb(y) to the time embedding before that SiLU (label_emb_linear_kernel, emb_gather_kernel).
#include "ops.h"

namespace {

__global__ void timestep_embedding_kernel(const float* t, int B, int dim, float max_period, float* out) {
  const int half = dim / 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * dim) return;
  const int b = idx / dim, j = idx % dim;
  float v = 0.f;  // zero pad when dim is odd (nn.py:113-114)
  if (j < 2 * half) {
    const int k = j < half ? j : j - half;
    // freqs = exp(-ln(max_period) * k / half), fp32 like the reference
    const float freq = expf(-logf(max_period) * (float)k / (float)half);
    const float arg = t[b] * freq;
    v = j < half ? cosf(arg) : sinf(arg);
  }
  out[idx] = v;
}

// out[b][j] = bias[j] + sum_k act(in[b][k]) * Wt[k][j].  One thread per (j, LR-row batch slab): the LR input rows
// are staged in LDS (broadcast reads), Wt reads are coalesced across lanes, 4 independent loads in flight.
constexpr int LB = 8;
constexpr int LIN_KB = 32;   // terms per block of the blocked summation (a multiple of 4)
template <int LR>
__device__ __forceinline__ void linear_rows(const float* xin, const float* __restrict__ Wt, const float* __restrict__ bias,
                                            float* __restrict__ out, int b0, int B, int K, int J, int j, int out_act) {
  // One fmaf chain over all of K rounds every step at the size of the running sum: at K = 2048 that is four to five times the error of the
  // reference's blocked fp32 GEMM and misses the op test's budget (tests/test_embed_ref_cpu.py).  Blocks of LIN_KB terms are summed in a chain of their own
  // and added to the total: K / LIN_KB + LIN_KB roundings at full size instead of K.
  float acc[LR];
#pragma unroll
  for (int r = 0; r < LR; ++r) acc[r] = 0.f;
  for (int kb = 0; kb < K; kb += LIN_KB) {
    const int ke = kb + LIN_KB < K ? kb + LIN_KB : K;
    float part[LR];
#pragma unroll
    for (int r = 0; r < LR; ++r) part[r] = 0.f;
    int k = kb;
    for (; k + 4 <= ke; k += 4) {
      const float w0 = Wt[(size_t)k * J + j], w1 = Wt[(size_t)(k + 1) * J + j];
      const float w2 = Wt[(size_t)(k + 2) * J + j], w3 = Wt[(size_t)(k + 3) * J + j];
#pragma unroll
      for (int r = 0; r < LR; ++r) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(xin + r * K + k);
        part[r] = fmaf(x[3], w3, fmaf(x[2], w2, fmaf(x[1], w1, fmaf(x[0], w0, part[r]))));
      }
    }
    for (; k < ke; ++k) {
      const float w = Wt[(size_t)k * J + j];
#pragma unroll
      for (int r = 0; r < LR; ++r) part[r] = fmaf(xin[r * K + k], w, part[r]);
    }
#pragma unroll
    for (int r = 0; r < LR; ++r) acc[r] += part[r];
  }
  const float bj = bias ? bias[j] : 0.f;
#pragma unroll
  for (int r = 0; r < LR; ++r) {
    const int b = b0 + r;
    if (b < B) {
      float v = acc[r] + bj;
      out[(size_t)b * J + j] = out_act ? silu_f<false>(v) : v;
    }
  }
}

__global__ void __launch_bounds__(128) linear_kernel(const float* __restrict__ in, const float* __restrict__ Wt,
                                                     const float* __restrict__ bias, float* __restrict__ out, int B, int K, int J,
                                                     int in_act, int out_act) {
  extern __shared__ float xin[];  // [LB][K]
  const int j = blockIdx.x * 128 + threadIdx.x;
  const int b0 = blockIdx.y * LB;
  for (int i = threadIdx.x; i < LB * K; i += 128) {
    const int r = i / K, k = i - r * K;
    float x = b0 + r < B ? in[(size_t)(b0 + r) * K + k] : 0.f;
    xin[i] = in_act ? silu_f<false>(x) : x;
  }
  __syncthreads();
  if (j >= J) return;
  linear_rows<LB>(xin, Wt, bias, out, b0, B, K, J, j, out_act);
}

// The error word of a handle is pinned host memory: a plain system-scope store (no read-modify-write over the bus); 2 = bad class label
__device__ __forceinline__ void flag_label_error(uint32_t* err) {
  if (err) __hip_atomic_store(err, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Class-conditional emb_layers: the linear_kernel contraction with a fused prologue that stages row r as
// silu(h[r / h_div] + label_emb[lab(r)]) - the time embedding (time_embed output, before the SiLU every emb_layers opens with) plus the
// label's embedding row, then that SiLU.  h_div = rows per time row (B for one shared step time, K for the sampler's (step, class) table).
template <int LR>
__global__ void __launch_bounds__(128) label_emb_linear_kernel(const float* __restrict__ h, int h_div, const float* __restrict__ lemb,
                                                               const int32_t* __restrict__ labels, int n_classes, const float* __restrict__ Wt,
                                                               const float* __restrict__ bias, float* __restrict__ out, int R, int K, int J,
                                                               uint32_t* err) {
  extern __shared__ float xin[];  // [LR][K]
  __shared__ int lab_s[LR];
  const int j = blockIdx.x * 128 + threadIdx.x;
  const int r0 = blockIdx.y * LR;
  if (threadIdx.x < LR) {
    const int r = r0 + threadIdx.x;
    int lab = -1;
    if (r < R) {
      lab = labels ? labels[r] : r % n_classes;
      if (lab < 0 || lab >= n_classes) {   // never read outside label_emb: the label term is zero, the handle is told
        if (blockIdx.x == 0) flag_label_error(err);
        lab = -1;
      }
    }
    lab_s[threadIdx.x] = lab;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < LR * K; i += 128) {
    const int rr = i / K, k = i - rr * K;
    const int r = r0 + rr;
    float x = 0.f;
    if (r < R) {
      const int lab = lab_s[rr];
      x = silu_f<false>(h[(size_t)(r / h_div) * K + k] + (lab >= 0 ? lemb[(size_t)lab * K + k] : 0.f));
    }
    xin[i] = x;
  }
  __syncthreads();
  if (j >= J) return;
  linear_rows<LR>(xin, Wt, bias, out, r0, R, K, J, j, 0);
}

// out[b] = table[labels[b]]: one thread per 16-byte quad of a row (a row's quads are adjacent threads: full-line loads and stores)
__global__ void __launch_bounds__(256) emb_gather_kernel(const float* __restrict__ table, const int32_t* __restrict__ labels, int n_classes,
                                                         float* __restrict__ out, int B, int J4, uint32_t* err) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)B * J4) return;
  const int b = (int)(idx / J4), q = (int)(idx - (size_t)b * J4);
  const int lab = labels[b];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
  if (lab >= 0 && lab < n_classes) v = *reinterpret_cast<const f32x4*>(table + ((size_t)lab * J4 + q) * 4);
  else if (q == 0) flag_label_error(err);
  *reinterpret_cast<f32x4*>(out + idx * 4) = v;
}

// Small-batch form (the sampler loops share one step time, so B = 1): a GEMV is latency-bound, so the K range is split
// over the 4 waves of a workgroup (lanes own 64 consecutive outputs, 8 independent loads in flight per lane) and the
// partial sums meet in LDS.
__global__ void __launch_bounds__(256) linear_small_kernel(const float* __restrict__ in, const float* __restrict__ Wt,
                                                           const float* __restrict__ bias, float* __restrict__ out, int B, int K, int J,
                                                           int in_act, int out_act) {
  __shared__ float part[4][LB][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + lane;
  const int kq = K / 4, k0 = wave * kq;
  float acc[LB];
#pragma unroll
  for (int r = 0; r < LB; ++r) acc[r] = 0.f;
  if (j < J) {
    for (int k = k0; k < k0 + kq; k += 8) {
      float w[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) w[u] = Wt[(size_t)(k + u) * J + j];
#pragma unroll
      for (int r = 0; r < LB; ++r) {
        if (r < B) {
#pragma unroll
          for (int u = 0; u < 8; ++u) {
            float x = in[(size_t)r * K + k + u];
            if (in_act) x = silu_f<false>(x);
            acc[r] = fmaf(x, w[u], acc[r]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int r = 0; r < LB; ++r) part[wave][r][lane] = acc[r];
  __syncthreads();
  if (wave == 0 && j < J) {
    const float bj = bias ? bias[j] : 0.f;
    for (int r = 0; r < B; ++r) {
      const float v = part[0][r][lane] + part[1][r][lane] + part[2][r][lane] + part[3][r][lane] + bj;
      out[(size_t)r * J + j] = out_act ? silu_f<false>(v) : v;
    }
  }
}

// One thread = one 16-byte channel fragment of one pixel (a pixel's fragments are adjacent threads: full-line NHWC stores; the
// NCHW reads of a channel are contiguous across the pixels of neighbouring thread groups).  Cpad is a multiple of the fragment.
template <typename T>
__global__ void __launch_bounds__(256) pack_nhwc_kernel(const float* x, int Cx, const float* cond, int Cc, int N, int HW, int Cpad, T* out) {
  constexpr int V = Elem<T>::VEC;
  const int G = Cpad / V;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (size_t)N * HW * G) return;
  const int g = idx % G;
  const size_t pix = idx / G;
  const int hw = pix % HW;
  const size_t n = pix / HW;
  float v[V];
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c = g * V + j;
    v[j] = c < Cx ? x[(n * Cx + c) * HW + hw] : (c < Cx + Cc ? cond[(n * Cc + (c - Cx)) * HW + hw] : 0.f);
  }
  *reinterpret_cast<u32x4*>(out + pix * Cpad + g * V) = float_to_frag(v, T());
}

template <typename T>
__global__ void unpack_nchw_kernel(const T* in, int N, int HW, int C, float* out) {
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)N * HW * C;
  if (idx >= total) return;
  const int hw = idx % HW;
  const size_t r = idx / HW;
  const int c = r % C;
  const size_t n = r / C;
  out[idx] = (float)in[(n * HW + hw) * C + c];
}

template <typename T>
__global__ void resample_kernel(const T* in, T* out, int N, int Hs, int Ws, int C, int mode) {
  const int Ho = mode == CONV_UP2 ? Hs * 2 : Hs / 2, Wo = mode == CONV_UP2 ? Ws * 2 : Ws / 2;
  const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)N * Ho * Wo * C;
  if (idx >= total) return;
  const int c = idx % C;
  size_t r = idx / C;
  const int x = r % Wo; r /= Wo;
  const int y = r % Ho;
  const size_t n = r / Ho;
  float v;
  if (mode == CONV_UP2) {
    v = (float)in[((n * Hs + (y >> 1)) * Ws + (x >> 1)) * C + c];
  } else {
    const size_t b = ((n * Hs + 2 * y) * Ws + 2 * x) * C + c;
    v = 0.25f * (((float)in[b] + (float)in[b + C]) + ((float)in[b + (size_t)Ws * C] + (float)in[b + (size_t)Ws * C + C]));
  }
  out[idx] = (T)v;
}

inline dim3 grid1d(size_t total, int block) { return dim3((unsigned)((total + block - 1) / block)); }

}  // namespace

int timestep_embedding_launch(const float* t, int B, int dim, float max_period, float* out, hipStream_t s) {
  hipLaunchKernelGGL(timestep_embedding_kernel, grid1d((size_t)B * dim, 256), dim3(256), 0, s, t, B, dim, max_period, out);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int linear_form(int B, int K) { return B <= LB && K % 32 == 0 ? 1 : 0; }

int label_emb_linear_form(int K) { return (size_t)16 * K * 4 <= 64 * 1024 ? 16 : LB; }

int linear_launch(const float* in, const float* Wt, const float* bias, float* out, int B, int K, int J, int in_act, int out_act,
                  hipStream_t s) {
  if (linear_form(B, K) == 1) {
    hipLaunchKernelGGL(linear_small_kernel, dim3((J + 63) / 64), dim3(256), 0, s, in, Wt, bias, out, B, K, J, in_act, out_act);
    MI355_CHECK_HIP(hipGetLastError());
    return 0;
  }
  dim3 grid((J + 127) / 128, (B + LB - 1) / LB);
  MI355_REQUIRE(K % 4 == 0 && (size_t)LB * K * 4 <= 64 * 1024, -4, "linear: K must be a multiple of 4 and <= 2048");
  hipLaunchKernelGGL(linear_kernel, grid, dim3(128), (size_t)LB * K * 4, s, in, Wt, bias, out, B, K, J, in_act, out_act);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int label_emb_linear_launch(const float* h, int h_div, const float* lemb, const int32_t* labels, int n_classes, const float* Wt,
                            const float* bias, float* out, int R, int K, int J, uint32_t* err, hipStream_t s) {
  MI355_REQUIRE(R > 0 && h_div > 0 && n_classes > 0, -1, "label_emb_linear: bad sizes");
  MI355_REQUIRE(K % 4 == 0 && (size_t)LB * K * 4 <= 64 * 1024, -4, "label_emb_linear: K must be a multiple of 4 and <= 2048");
  // 16-row slabs halve the weight re-reads of the per-step form (B rows) where they fit the LDS budget of linear_kernel
  if (label_emb_linear_form(K) == 16) {
    hipLaunchKernelGGL(label_emb_linear_kernel<16>, dim3((J + 127) / 128, (R + 15) / 16), dim3(128), (size_t)16 * K * 4, s, h, h_div, lemb,
                       labels, n_classes, Wt, bias, out, R, K, J, err);
  } else {
    hipLaunchKernelGGL(label_emb_linear_kernel<LB>, dim3((J + 127) / 128, (R + LB - 1) / LB), dim3(128), (size_t)LB * K * 4, s, h, h_div, lemb,
                       labels, n_classes, Wt, bias, out, R, K, J, err);
  }
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int emb_gather_launch(const float* table, const int32_t* labels, int n_classes, float* out, int B, int J, uint32_t* err, hipStream_t s) {
  MI355_REQUIRE(table && labels && out && B > 0 && n_classes > 0, -1, "emb_gather: bad argument");
  MI355_REQUIRE(J % 4 == 0 && (reinterpret_cast<uintptr_t>(table) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0, -2,
                "emb_gather: rows must be whole 16-byte vectors");
  hipLaunchKernelGGL(emb_gather_kernel, grid1d((size_t)B * (J / 4), 256), dim3(256), 0, s, table, labels, n_classes, out, B, J / 4, err);
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int pack_nhwc_launch(int dtype, const float* x, int Cx, const float* cond, int Cc, int N, int HW, int Cpad, void* out,
                     hipStream_t s) {
  const int V = dtype == 0 ? 4 : 8;
  MI355_REQUIRE(Cpad % V == 0, -2, "pack_nhwc: padded channels must be whole 16-byte fragments");
  const size_t total = (size_t)N * HW * (Cpad / V);
  dispatch_dtype(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(pack_nhwc_kernel<T>, grid1d(total, 256), dim3(256), 0, s, x, Cx, cond, Cc, N, HW, Cpad, (T*)out); return 0; });
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int unpack_nchw_launch(int dtype, const void* in, int N, int HW, int C, float* out, hipStream_t s) {
  const size_t total = (size_t)N * HW * C;
  dispatch_dtype(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(unpack_nchw_kernel<T>, grid1d(total, 256), dim3(256), 0, s, (const T*)in, N, HW, C, out); return 0; });
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}

int resample_launch(int dtype, const void* in, void* out, int N, int Hs, int Ws, int C, int mode, hipStream_t s) {
  const int Ho = mode == CONV_UP2 ? Hs * 2 : Hs / 2, Wo = mode == CONV_UP2 ? Ws * 2 : Ws / 2;
  const size_t total = (size_t)N * Ho * Wo * C;
  dispatch_dtype(dtype, [&](auto t) { using T = decltype(t); hipLaunchKernelGGL(resample_kernel<T>, grid1d(total, 256), dim3(256), 0, s, (const T*)in, (T*)out, N, Hs, Ws, C, mode); return 0; });
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
