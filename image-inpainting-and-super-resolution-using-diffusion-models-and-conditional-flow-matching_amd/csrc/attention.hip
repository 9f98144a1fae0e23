// Fused QK^T -> fp32 softmax -> PV (flash-style, online softmax) for the U-Net's AttentionBlock.
//
// Reference: QKVAttentionLegacy.forward (AD/image_diffusion/unet.py:433-448) and QKVAttention.forward
// (:464-483): w = softmax_s((q*s)^T (k*s)), s = ch^-1/4, softmax in fp32; a = w v.  The reference
// materialises the [B*heads, T, T] weight matrix in HBM; here it never leaves registers.
//
// Layout: qkv is NHWC [N][T][3C] (the qkv 1x1 conv's output), channel order as in the reference
// (legacy: per head [q|k|v]; new: [all q | all k | all v]).  out is NHWC [N][T][C].
// One workgroup = 4 waves x QB blocks of 16 query rows of one (image, head).  Per KT-key tile:
//   S^T = K Q^T    (keys on MFMA rows, queries on the lane -> the softmax column is lane-local + 2 shuffles)
//   O^T += V^T P^T (P^T is already the B operand, straight from the S^T accumulators)
// K and V tiles are staged ROW-MAJOR ([key][channel], 16-byte copies, rows padded by 32 B): K is read by rows
// (ds_read_b128), V^T comes out of the same kind of image through the hardware transpose read ds_read_b64_tr_b16
// (bf16; 4 keys x 16 channels per 16-lane group, conflict-free with the 32-byte row pad) - no transposing stores.
// Tiles are double-buffered (NBUF = 2): the next tile's global loads are issued right after the barrier that publishes
// the current one and written to the other buffer after the tile's MFMAs, so there is ONE barrier per key tile and the
// load latency hides behind the compute.  Head sizes up to 512 channels (torchcfm's default single head at 384 / 512
// channels, mnist/train_mnist_hy.py:312-318) use 32-key tiles (and, in fp32, a single buffer) to stay inside 160 KB.
// The fragment loops, the softmax, the transposed read, the store and the staging rule are attn_core.h's.
#include "ops.h"
#include "attn_core.h"

namespace {

struct AttnKArgs {
  const void* qkv; void* out;
  int N, T, heads, C;
  int qoff_h, koff, voff;  // channel offsets: q of head h at h*qoff_h, k at koff + h*qoff_h, v at voff + h*qoff_h
  float scale2;
};

// Register budget: with a 512-register budget (one workgroup per CU) the compiler puts the MFMA accumulators into AccVGPRs, and the
// softmax / rescale between the two GEMMs then costs a v_accvgpr_read or _write per accumulator register and key tile (192 of them
// beside 32 MFMAs at 64 channels).  Promising two workgroups per CU caps the budget at 256 = the VGPR form of the MFMAs, no copies;
// the head sizes whose accumulators need more than that keep the full budget.
template <typename T, int CH, int QB>
constexpr int attn_min_blocks() { return (sizeof(T) == 2 ? CH * QB <= 192 : CH <= 96) ? 2 : 1; }

template <typename T, int CH, int QB, int KT, int NBUF>
__global__ void __launch_bounds__(256, (attn_min_blocks<T, CH, QB>())) attention_kernel(AttnKArgs p) {
  using E = Elem<T>;
  constexpr int V = E::VEC, CHUNK = E::CHUNK, SZ = sizeof(T);
  constexpr int KST = CH / CHUNK;           // k-steps over channels for S^T
  constexpr int CI = CH / 16;               // 16-channel row tiles of O^T
  constexpr int MT = KT / 16;               // 16-key row tiles of S^T per key tile
  constexpr int ROW = CH * SZ + 32;         // K / V tile row stride (bytes)
  constexpr int TILE = KT * ROW;            // bytes of one K (or V) tile
  constexpr int NF = attn_stage_frags<T, CH, KT>();   // 16-B fragments per thread per tile (K and V each)
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [NBUF][K tile | V tile]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const int n = blockIdx.y / p.heads, h = blockIdx.y % p.heads;
  const int q0 = blockIdx.x * (64 * QB) + wave * (16 * QB);
  const size_t rowstride = (size_t)3 * p.C;
  const T* base = reinterpret_cast<const T*>(p.qkv) + (size_t)n * p.T * rowstride;
  const int qc = h * p.qoff_h, kc = p.koff + h * p.qoff_h, vc = p.voff + h * p.qoff_h;
  const float c2 = p.scale2 * 1.4426950408889634f;

  // Q^T fragments (B operand): lane holds Q[q0 + 16 qb + lr][ks*CHUNK + lq*V .. +V)
  u32x4 qf[QB][KST];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int ks = 0; ks < KST; ++ks) {
      const int q = q0 + 16 * qb + lr;
      qf[qb][ks] = u32x4{0u, 0u, 0u, 0u};
      if (q < p.T) qf[qb][ks] = *reinterpret_cast<const u32x4*>(base + (size_t)q * rowstride + qc + ks * CHUNK + lq * V);
      // q carries ch^-1/2 * log2(e) from here on: S^T comes out of the MFMAs in the log2 domain and the softmax needs no multiply
      // per element (fp32: exact to rounding; bf16: one more rounding of q, the size of the one the qkv conv's store already made)
      float f[V];
      frag_to_float(qf[qb][ks], f, T());
#pragma unroll
      for (int j = 0; j < V; ++j) f[j] *= c2;
      qf[qb][ks] = float_to_frag(f, T());
    }

  f32x4 o[QB][CI];
  float m_run[QB], l_run[QB];
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    m_run[qb] = 0.f; l_run[qb] = 0.f;
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) o[qb][ci] = f32x4{0.f, 0.f, 0.f, 0.f};
  }

  // ---- staging: thread owns fragments e = tid + 256 u of a tile (row e / FPR, 16-B slot e % FPR), K and V alike; loads and LDS writes
  //      apart.  The load half is attn_stage_rows_load's rule in this kernel's own text: on the shared form attention_kernel<float, 512, 1,
  //      32, 1>, which sits at the 512-register limit, spills 16 registers instead of 12 (profiles/attn_core_parity.md) ----
  constexpr int FPR = CH / V;               // 16-B fragments per row
  u32x4 kreg[NF], vreg[NF];
  auto load_tile = [&](int kt) {
#pragma unroll
    for (int u = 0; u < NF; ++u) {
      const int e = tid + 256 * u, s = e / FPR, f = e - s * FPR;
      const int key = kt * KT + s;
      kreg[u] = u32x4{0u, 0u, 0u, 0u}; vreg[u] = u32x4{0u, 0u, 0u, 0u};
      if (e < KT * FPR && key < p.T) {
        const T* rp = base + (size_t)key * rowstride;
        kreg[u] = *reinterpret_cast<const u32x4*>(rp + kc + f * V);
        vreg[u] = *reinterpret_cast<const u32x4*>(rp + vc + f * V);
      }
    }
  };
  auto store_tile = [&](int buf) { attn_stage_rows_store<T, CH, KT>(smem + buf * (2 * TILE), smem + buf * (2 * TILE) + TILE, kreg, vreg, tid); };

  const int ntiles = (p.T + KT - 1) / KT;
  load_tile(0);
  store_tile(0);
  for (int kt = 0; kt < ntiles; ++kt) {
    const int buf = NBUF == 2 ? (kt & 1) : 0;
    __syncthreads();                        // tile kt is staged (and, NBUF == 2, every wave is done with tile kt - 1's buffer)
    if (NBUF == 2 && kt + 1 < ntiles) load_tile(kt + 1);   // in flight during this tile's MFMAs
    const char* klds = smem + buf * (2 * TILE);
    const char* vlds = klds + TILE;

    // ---- S^T = K Q^T : MT row tiles of 16 keys; a K fragment is read once and used by all QB query blocks ----
    f32x4 sacc[QB][MT];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int mi = 0; mi < MT; ++mi) sacc[qb][mi] = f32x4{-m_run[qb], -m_run[qb], -m_run[qb], -m_run[qb]};   // the column's reference offset
    attn_scores<T, ROW, MT, KST, QB>(sacc, klds, qf, lr, lq);
    // ---- online softmax over keys (column = query = lane&15; rows spread over regs and lane>>4), offset-in-accumulator form ----
    if ((kt + 1) * KT > p.T) {              // only a ragged last tile has keys to mask (wave-uniform)
#pragma unroll
      for (int qb = 0; qb < QB; ++qb)
#pragma unroll
        for (int mi = 0; mi < MT; ++mi)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (kt * KT + mi * 16 + lq * 4 + r >= p.T) sacc[qb][mi][r] = -INFINITY;
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) attn_softmax_offset<MT, CI>(sacc[qb], o[qb], m_run[qb], l_run[qb], kt == 0);
    attn_pv<T, ROW, MT, CI, QB>(o, sacc, vlds, lr, lq);   // O^T += V^T P^T
    if (kt + 1 < ntiles) {
      if (NBUF == 2) store_tile((kt + 1) & 1);   // the other buffer: last read during tile kt - 1, before this tile's barrier
      else { __syncthreads(); load_tile(kt + 1); store_tile(0); }
    }
  }
  // ---- normalise and store: lane holds channels ci*16 + 4*lq + r of query q0 + 16 qb + lr ----
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int q = q0 + 16 * qb + lr;
    attn_store_normalised<T, CI>(reinterpret_cast<T*>(p.out) + ((size_t)n * p.T + q) * p.C + h * CH, q < p.T, o[qb], l_run[qb], lq);
  }
}

template <typename T, int CH, int QB, int KT, int NBUF>
int launch_one(const AttnKArgs& a, hipStream_t s) {
  auto kern = attention_kernel<T, CH, QB, KT, NBUF>;
  constexpr size_t lds = (size_t)NBUF * 2 * KT * (CH * sizeof(T) + 32);
  static_assert(lds <= 160 * 1024, "attention tile does not fit the LDS");
  if (lds > 64 * 1024) { if (int rc = mi355_allow_big_lds(kern, "attention")) return rc; }
  dim3 grid((a.T + 64 * QB - 1) / (64 * QB), a.N * a.heads);
  hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, a);
  return 0;
}

template <typename T>
int launch_attn(const AttnKArgs& a, int ch, hipStream_t s) {
  constexpr bool F32 = sizeof(T) == 4;
  // two query blocks per wave (128 queries per workgroup: half the K/V staging per query) once the sequence is long enough
  const bool wide = a.T >= 256;
  switch (ch) {
    case 32: return wide ? launch_one<T, 32, 2, 64, 2>(a, s) : launch_one<T, 32, 1, 64, 2>(a, s);
    case 64: return wide ? launch_one<T, 64, 2, 64, 2>(a, s) : launch_one<T, 64, 1, 64, 2>(a, s);
    case 96: return launch_one<T, 96, 1, 64, 2>(a, s);
    case 128: return launch_one<T, 128, 1, 64, 2>(a, s);
    case 192: return launch_one<T, 192, 1, 32, 2>(a, s);
    case 256: return launch_one<T, 256, 1, 32, 2>(a, s);
    case 384: return launch_one<T, 384, 1, 32, F32 ? 1 : 2>(a, s);
    case 512: return launch_one<T, 512, 1, 32, F32 ? 1 : 2>(a, s);
    default: break;
  }
  mi355_set_error("attention: head channels must be one of 32, 64, 96, 128, 192, 256, 384, 512 (got " + std::to_string(ch) + ")");
  return -4;
}

}  // namespace

int attention_launch(const AttnDesc& d, hipStream_t stream) {
  AttnKArgs a;
  a.qkv = d.qkv; a.out = d.out; a.N = d.N; a.T = d.T; a.heads = d.heads; a.C = d.heads * d.ch;
  const AttnChannelOffsets co = attn_channel_offsets(d.new_order, d.ch, a.C);
  a.qoff_h = co.qoff_h; a.koff = co.koff; a.voff = co.voff; a.scale2 = co.scale2;
  int rc = dispatch_dtype(d.dtype, [&](auto t) { return launch_attn<decltype(t)>(a, d.ch, stream); });
  if (rc) return rc;
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
