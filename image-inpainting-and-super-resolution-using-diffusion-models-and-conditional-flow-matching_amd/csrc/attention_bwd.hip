// Backward of the attention core (QKVAttentionLegacy / QKVAttention, AD/image_diffusion/unet.py:433-448, 464-483) for the
// reconstruction-guidance data gradient:   S = scale2 Q K^T, P = softmax_rows(S), A = P V
//   dV = P^T dA,  dP = dA V^T,  dS = P o (dP - D),  D_q = dA_q . A_q,  dQ = scale2 dS K,  dK = scale2 dS^T Q
// Flash-style, nothing of size T x T is stored; two kernels that mirror the forward's structure (attention.hip):
//   attention_bwd_q   workgroup = 64 queries of one (image, head): pass 1 over the key tiles rebuilds the softmax statistics
//                     L = m + log2(l) (log2 domain), pass 2 forms dS^T = P^T o (V dA^T - D) and accumulates dQ^T += K^T dS^T;
//                     also writes L and D per query for the second kernel;
//   attention_bwd_kv  workgroup = 64 keys: streams (Q, dA) tiles, S = Q K^T with the keys on the lane, dV^T += dA^T P,
//                     dK^T += Q^T dS - the accumulator tiles are the next MFMA's B operand as they stand (their rows, the
//                     queries, are the summed index), Q^T / dA^T come through the transposed LDS read.
// qkv / dqkv: NHWC [N][T][3C] in the reference's channel order; a, da: [N][T][C]; L, D: fp32 [N * heads][T].
// The fragment loops, the transposed operand read, the accumulator pack, the gradient stores and the tile staging are attn_core.h's; its
// primitives take QB column blocks per wave, these kernels have one: the [1] of their fragment and accumulator arrays.
#include "ops.h"
#include "attn_core.h"

namespace {

struct AttnBwdArgs {
  const void* qkv; const void* a; const void* da; void* dqkv;
  float* L; float* D;
  int N, T, heads, C;
  int qoff_h, koff, voff;
  float scale2;
};

// Register budget as in attention.hip (attn_min_blocks): two workgroups per CU = a 256-register budget = MFMAs in their VGPR form, no
// v_accvgpr copies around the softmax; the head sizes whose live set needs more keep the full budget.
template <typename T, int CH> constexpr int bwd_q_min_blocks() { return (sizeof(T) == 2 ? CH <= 192 : CH <= 96) ? 2 : 1; }
template <typename T, int CH> constexpr int bwd_kv_min_blocks() { return (sizeof(T) == 2 ? CH <= 128 : CH <= 64) ? 2 : 1; }

// ---- dQ (+ L, D) ----------------------------------------------------------------------------------------------------------------
template <typename T, int CH>
__global__ void __launch_bounds__(256, (bwd_q_min_blocks<T, CH>())) attention_bwd_q_kernel(AttnBwdArgs p) {
  using E = Elem<T>;
  constexpr int V = E::VEC, CHUNK = E::CHUNK, SZ = sizeof(T);
  constexpr int KST = CH / CHUNK, CI = CH / 16, KT = 64, MT = 4;
  constexpr int ROW = CH * SZ + 32, TILE = KT * ROW, NF = attn_stage_frags<T, CH, KT>();
  extern __shared__ __attribute__((aligned(16))) char smem[];   // K tile | V tile
  char* klds = smem; char* vlds = smem + TILE;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int n = blockIdx.y / p.heads, h = blockIdx.y % p.heads;
  const int q = blockIdx.x * 64 + wave * 16 + lr;
  const bool qok = q < p.T;
  const size_t rs = (size_t)3 * p.C;
  const T* base = reinterpret_cast<const T*>(p.qkv) + (size_t)n * p.T * rs;
  const int qc = h * p.qoff_h, kc = p.koff + h * p.qoff_h, vc = p.voff + h * p.qoff_h;
  const T* arow = reinterpret_cast<const T*>(p.a) + ((size_t)n * p.T + (qok ? q : 0)) * p.C + h * CH;
  const T* drow = reinterpret_cast<const T*>(p.da) + ((size_t)n * p.T + (qok ? q : 0)) * p.C + h * CH;

  u32x4 qf[1][KST], df[1][KST];
  float dsum = 0.f;
#pragma unroll
  for (int ks = 0; ks < KST; ++ks) {
    qf[0][ks] = u32x4{0u, 0u, 0u, 0u}; df[0][ks] = u32x4{0u, 0u, 0u, 0u};
    if (qok) {
      qf[0][ks] = *reinterpret_cast<const u32x4*>(base + (size_t)q * rs + qc + ks * CHUNK + lq * V);
      df[0][ks] = *reinterpret_cast<const u32x4*>(drow + ks * CHUNK + lq * V);
      float fa[V], fd[V];
      frag_to_float(*reinterpret_cast<const u32x4*>(arow + ks * CHUNK + lq * V), fa, T());
      frag_to_float(df[0][ks], fd, T());
#pragma unroll
      for (int j = 0; j < V; ++j) dsum += fa[j] * fd[j];
    }
  }
  dsum += __shfl_xor(dsum, 16);
  dsum += __shfl_xor(dsum, 32);            // D_q = dA_q . A_q, identical in the four lanes of a query column

  auto stage = [&](int kt) {
    u32x4 kreg[NF], vreg[NF];
    attn_stage_rows_load<T, CH, KT>(kreg, vreg, base + kc, rs, base + vc, rs, kt * KT, p.T, tid);
    attn_stage_rows_store<T, CH, KT>(klds, vlds, kreg, vreg, tid);
  };
  auto scores = [&](int kt, f32x4 (&sacc)[1][MT]) {   // S^T tile (raw q.k), -inf on keys past the end
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) sacc[0][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    attn_scores<T, ROW, MT, KST, 1>(sacc, klds, qf, lr, lq);
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) if (kt * KT + mi * 16 + lq * 4 + r >= p.T) sacc[0][mi][r] = -INFINITY;
  };
  const int ntiles = (p.T + KT - 1) / KT;
  const float c2 = p.scale2 * 1.4426950408889634f;
  // ---- pass 1: softmax statistics.  Its own form, not attn_softmax_offset: there is no O to rescale and q is unscaled here (pass 2 and the
  //      second kernel need the raw S for exp2(S c2 - L)), so the statistics are the classic running (max, sum) with m_run = -inf ----
  float m_run = -INFINITY, l_run = 0.f;
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage(kt);
    __syncthreads();
    f32x4 sacc[1][MT];
    scores(kt, sacc);
    float mx = -INFINITY;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sacc[0][mi][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx * c2);
    float psum = 0.f;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) psum += __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[0][mi][r], c2, -m_new));
    l_run = l_run * __builtin_amdgcn_exp2f(m_run - m_new) + psum;
    m_run = m_new;
  }
  l_run += __shfl_xor(l_run, 16);
  l_run += __shfl_xor(l_run, 32);
  const float Lq = m_run + log2f(l_run);
  if (qok && lq == 0) { p.L[(size_t)blockIdx.y * p.T + q] = Lq; p.D[(size_t)blockIdx.y * p.T + q] = dsum; }
  // ---- pass 2: dQ^T += K^T dS^T ----
  f32x4 dq[1][CI];
#pragma unroll
  for (int ci = 0; ci < CI; ++ci) dq[0][ci] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int kt = 0; kt < ntiles; ++kt) {
    __syncthreads();
    stage(kt);
    __syncthreads();
    f32x4 sacc[1][MT], dp[1][MT];
    scores(kt, sacc);
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) dp[0][mi] = f32x4{0.f, 0.f, 0.f, 0.f};
    attn_scores<T, ROW, MT, KST, 1>(dp, vlds, df, lr, lq);   // dP^T = V dA^T
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(sacc[0][mi][r], c2, -Lq));   // 0 on masked keys
        sacc[0][mi][r] = pr * (dp[0][mi][r] - dsum) * p.scale2;                              // dS^T (the S scale folded in)
      }
    attn_pv<T, ROW, MT, CI, 1>(dq, sacc, klds, lr, lq);
  }
  if (qok) attn_store_quads<T, CI>(reinterpret_cast<T*>(p.dqkv) + ((size_t)n * p.T + q) * rs + qc, dq[0], 1.0f, lq);
}

// ---- dK, dV -------------------------------------------------------------------------------------------------------------------------
template <typename T, int CH>
__global__ void __launch_bounds__(256, (bwd_kv_min_blocks<T, CH>())) attention_bwd_kv_kernel(AttnBwdArgs p) {
  using E = Elem<T>;
  constexpr int V = E::VEC, CHUNK = E::CHUNK, SZ = sizeof(T);
  constexpr int KST = CH / CHUNK, CI = CH / 16, QT = 64, MT = 4;
  constexpr int ROW = CH * SZ + 32, TILE = QT * ROW, FPR = CH / V, NF = (QT * FPR + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // Q tile | dA tile | L[64] | D[64]
  char* qlds = smem; char* dlds = smem + TILE;
  float* Ll = reinterpret_cast<float*>(smem + 2 * TILE); float* Dl = Ll + QT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int n = blockIdx.y / p.heads, h = blockIdx.y % p.heads;
  const int key = blockIdx.x * 64 + wave * 16 + lr;
  const bool kok = key < p.T;
  const size_t rs = (size_t)3 * p.C;
  const T* base = reinterpret_cast<const T*>(p.qkv) + (size_t)n * p.T * rs;
  const T* dab = reinterpret_cast<const T*>(p.da) + (size_t)n * p.T * p.C + h * CH;
  const int qc = h * p.qoff_h, kc = p.koff + h * p.qoff_h, vc = p.voff + h * p.qoff_h;
  u32x4 kf[1][KST], vf[1][KST];
#pragma unroll
  for (int ks = 0; ks < KST; ++ks) {
    kf[0][ks] = u32x4{0u, 0u, 0u, 0u}; vf[0][ks] = u32x4{0u, 0u, 0u, 0u};
    if (kok) {
      kf[0][ks] = *reinterpret_cast<const u32x4*>(base + (size_t)key * rs + kc + ks * CHUNK + lq * V);
      vf[0][ks] = *reinterpret_cast<const u32x4*>(base + (size_t)key * rs + vc + ks * CHUNK + lq * V);
    }
  }
  f32x4 dk[1][CI], dv[1][CI];
#pragma unroll
  for (int ci = 0; ci < CI; ++ci) { dk[0][ci] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[0][ci] = f32x4{0.f, 0.f, 0.f, 0.f}; }
  const float c2 = p.scale2 * 1.4426950408889634f;
  const int ntiles = (p.T + QT - 1) / QT;
  for (int qt = 0; qt < ntiles; ++qt) {
    __syncthreads();
    {   // stage the query tile: Q and dA rows (zero past the end), L (+inf past the end: P = 0) and D.  attn_stage_rows' rule in this kernel's
        // own text: attention_bwd_kv_kernel<float, 256> sits at the 512-register limit and spills 23 registers on the shared form, 18 at
        // the parent, 6 like this (profiles/attn_core_parity.md)
      u32x4 qreg[NF], dreg[NF];
#pragma unroll
      for (int u = 0; u < NF; ++u) {
        const int e = tid + 256 * u, s = e / FPR, f = e - s * FPR, q = qt * QT + s;
        qreg[u] = u32x4{0u, 0u, 0u, 0u}; dreg[u] = u32x4{0u, 0u, 0u, 0u};
        if (e < QT * FPR && q < p.T) {
          qreg[u] = *reinterpret_cast<const u32x4*>(base + (size_t)q * rs + qc + f * V);
          dreg[u] = *reinterpret_cast<const u32x4*>(dab + (size_t)q * p.C + f * V);
        }
      }
#pragma unroll
      for (int u = 0; u < NF; ++u) {
        const int e = tid + 256 * u, s = e / FPR, f = e - s * FPR;
        if (e < QT * FPR) { *reinterpret_cast<u32x4*>(qlds + s * ROW + f * 16) = qreg[u]; *reinterpret_cast<u32x4*>(dlds + s * ROW + f * 16) = dreg[u]; }
      }
      if (tid < QT) {
        const int q = qt * QT + tid;
        Ll[tid] = q < p.T ? p.L[(size_t)blockIdx.y * p.T + q] : INFINITY;
        Dl[tid] = q < p.T ? p.D[(size_t)blockIdx.y * p.T + q] : 0.f;
      }
    }
    __syncthreads();
    // S = Q K^T and dP = dA V^T: rows = queries (registers / lane >> 4), columns = this wave's keys (lane & 15)
    f32x4 pt[1][MT], ds[1][MT];
#pragma unroll
    for (int mi = 0; mi < MT; ++mi) { pt[0][mi] = f32x4{0.f, 0.f, 0.f, 0.f}; ds[0][mi] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    attn_scores<T, ROW, MT, KST, 1>(pt, qlds, kf, lr, lq);
    attn_scores<T, ROW, MT, KST, 1>(ds, dlds, vf, lr, lq);
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = mi * 16 + lq * 4 + r;
        const float pr = __builtin_amdgcn_exp2f(__builtin_fmaf(pt[0][mi][r], c2, -Ll[row]));
        pt[0][mi][r] = pr;
        ds[0][mi][r] = pr * (ds[0][mi][r] - Dl[row]) * p.scale2;
      }
    attn_pv<T, ROW, MT, CI, 1>(dv, pt, dlds, lr, lq);   // dV^T += dA^T P
    attn_pv<T, ROW, MT, CI, 1>(dk, ds, qlds, lr, lq);   // dK^T += Q^T dS
  }
  if (kok) {
    T* orow = reinterpret_cast<T*>(p.dqkv) + ((size_t)n * p.T + key) * rs;
    attn_store_quads<T, CI>(orow + kc, dk[0], 1.0f, lq);
    attn_store_quads<T, CI>(orow + vc, dv[0], 1.0f, lq);
  }
}

template <typename T, int CH>
int launch_bwd(const AttnBwdArgs& a, hipStream_t s) {
  constexpr size_t tile = (size_t)64 * (CH * sizeof(T) + 32);
  constexpr size_t lds_q = 2 * tile, lds_kv = 2 * tile + 2 * 64 * sizeof(float);
  static_assert(lds_kv <= 160 * 1024, "attention backward tile does not fit the LDS");
  auto kq = attention_bwd_q_kernel<T, CH>;
  auto kkv = attention_bwd_kv_kernel<T, CH>;
  if (lds_q > 64 * 1024) { if (int rc = mi355_allow_big_lds(kq, "attention backward")) return rc; }
  if (lds_kv > 64 * 1024) { if (int rc = mi355_allow_big_lds(kkv, "attention backward")) return rc; }
  dim3 grid((a.T + 63) / 64, a.N * a.heads);
  hipLaunchKernelGGL(kq, grid, dim3(256), lds_q, s, a);
  hipLaunchKernelGGL(kkv, grid, dim3(256), lds_kv, s, a);
  return 0;
}

template <typename T>
int launch_bwd_ch(const AttnBwdArgs& a, int ch, hipStream_t s) {
  switch (ch) {
    case 32: return launch_bwd<T, 32>(a, s);
    case 64: return launch_bwd<T, 64>(a, s);
    case 96: return launch_bwd<T, 96>(a, s);
    case 128: return launch_bwd<T, 128>(a, s);
    case 192: return launch_bwd<T, 192>(a, s);
    case 256: return launch_bwd<T, 256>(a, s);
    default: break;
  }
  mi355_set_error("attention backward: head channels must be one of 32, 64, 96, 128, 192, 256 (got " + std::to_string(ch) + ")");
  return -4;
}

}  // namespace

int attention_bwd_launch(const AttnBwdDesc& d, hipStream_t stream) {
  MI355_REQUIRE(d.qkv && d.a && d.da && d.dqkv && d.L && d.D, -1, "attention backward: null argument");
  MI355_REQUIRE(d.dtype == DT_F32 || d.dtype == DT_BF16, -4, "attention backward: element type must be fp32 or bf16");
  AttnBwdArgs a;
  a.qkv = d.qkv; a.a = d.a; a.da = d.da; a.dqkv = d.dqkv; a.L = d.L; a.D = d.D;
  a.N = d.N; a.T = d.T; a.heads = d.heads; a.C = d.heads * d.ch;
  const AttnChannelOffsets co = attn_channel_offsets(d.new_order, d.ch, a.C);
  a.qoff_h = co.qoff_h; a.koff = co.koff; a.voff = co.voff; a.scale2 = co.scale2;
  int rc = d.dtype == 0 ? launch_bwd_ch<float>(a, d.ch, stream) : launch_bwd_ch<bf16>(a, d.ch, stream);
  if (rc) return rc;
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
