// The attention core: the device code the five attention kernels share (attention.hip, attn_fused.hip, attention_bwd.hip).
//
// All of them work on the same picture.  A wave owns 16-column blocks of a 16x16 MFMA tile grid: column = lane & 15 (lr) = a query (forward,
// backward dQ) or a key (backward dK / dV); the accumulator rows 4 (lane >> 4) + r (lq, r) = the index that the NEXT product sums over, so an
// accumulator tile is that product's B operand as it stands.  The A operands come from ROW-MAJOR LDS tiles ([row][channel], row stride ROW
// bytes = the channels + a 32-byte pad): read by rows (ds_read_b128) for S^T = K Q^T, and through the hardware transpose read
// ds_read_b64_tr_b16 (two-byte elements) or a four-row gather (fp32) for O^T += V^T P^T.
//
// Device __forceinline__ templates only.  Every primitive takes the caller's registers by reference and the lane's (lr, lq); none of them
// holds a barrier, none knows what the tile is (K, V, Q or dA) or where it came from.
#pragma once
#include "common.h"

typedef short s16x4 __attribute__((ext_vector_type(4)));

// A^T-operand fragment of a row-major LDS tile: channels 16 ci + (lane & 15) as MFMA rows, 8 (two-byte) / 4 (fp32) tile rows as the k index,
// in the k order of the B fragments attn_acc_frag builds (two-byte: rows r0 + 4 lq + {0..3} and r0 + 16 + 4 lq + {0..3}; fp32: rows
// r0 + 4 lq + {0..3}).  Two-byte: lane 4q + p of a 16-lane group addresses row q, columns 4p .. 4p + 3 of a 4-row x 16-channel block and
// receives column (lane & 15) of its 4 rows (conflict-free with the 32-byte row pad; EXEC must be all ones).
template <typename T, int ROW>
__device__ __forceinline__ u32x4 attn_tr_frag(const char* tile, int r0, int ci, int lr, int lq) {
  if constexpr (Elem<T>::DTYPE == 1) {
    const char* vrow = tile + (r0 + 4 * lq + (lr >> 2)) * ROW + 8 * (lr & 3) + ci * 32;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vrow));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vrow + 16 * ROW));
    const u32x2 l2 = __builtin_bit_cast(u32x2, lo), h2 = __builtin_bit_cast(u32x2, hi);
    return u32x4{l2[0], l2[1], h2[0], h2[1]};
  } else {
    const char* vp = tile + (r0 + 4 * lq) * ROW + (16 * ci + lr) * 4;
    return u32x4{*reinterpret_cast<const uint32_t*>(vp), *reinterpret_cast<const uint32_t*>(vp + ROW),
                 *reinterpret_cast<const uint32_t*>(vp + 2 * ROW), *reinterpret_cast<const uint32_t*>(vp + 3 * ROW)};
  }
}
// B fragment (k = the accumulator tiles' row index) from two (two-byte elements) or one (fp32: t1 is not read) 16x16 accumulator tiles.
// Rounding: pack4 = one RNE conversion per element, `(bf16)x` for bf16 and `(f16)x` for f16 - the same conversion the backward kernels used
// to spell as a bf16x8 of `(bf16)` casts, so one form serves the forward (bf16, f16) and the backward (bf16); fp32 is a bit copy.
template <typename T>
__device__ __forceinline__ u32x4 attn_acc_frag(const f32x4& t0, const f32x4& t1) {
  if constexpr (Elem<T>::DTYPE == 1) {
    const u32x2 p0 = pack4(t0, T()), p1 = pack4(t1, T());
    return u32x4{p0[0], p0[1], p1[0], p1[1]};
  } else {
    return __builtin_bit_cast(u32x4, t0);
  }
}
template <typename T> constexpr int attn_frag_tiles() { return Elem<T>::DTYPE == 1 ? 2 : 1; }   // accumulator tiles per B fragment

// sacc[qb][mi] += tile rows 16 mi .. + 15 (MFMA rows) x bfrag[qb] (columns), summed over KST channel steps.  The caller sets the start values
// (zero, or minus a column's running softmax offset) and masks afterwards; a tile fragment is read once and used by all QB column blocks.
template <typename T, int ROW, int MT, int KST, int QB>
__device__ __forceinline__ void attn_scores(f32x4 (&sacc)[QB][MT], const char* tile, const u32x4 (&bfrag)[QB][KST], int lr, int lq) {
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int ks = 0; ks < KST; ++ks) {
      const u32x4 af = *reinterpret_cast<const u32x4*>(tile + (mi * 16 + lr) * ROW + (ks * 4 + lq) * 16);
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) mma16(sacc[qb][mi], af, bfrag[qb][ks], T());
    }
}

// the maximum over the four lanes that share a column: two VALU row swaps (v_permlane16_swap / v_permlane32_swap), no LDS round trip
__device__ __forceinline__ float attn_colmax(float v) {
  const auto s16 = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(uint32_t, v), __builtin_bit_cast(uint32_t, v), false, false);
  v = fmaxf(__builtin_bit_cast(float, (uint32_t)s16[0]), __builtin_bit_cast(float, (uint32_t)s16[1]));
  const auto s32 = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(uint32_t, v), __builtin_bit_cast(uint32_t, v), false, false);
  return fmaxf(__builtin_bit_cast(float, (uint32_t)s32[0]), __builtin_bit_cast(float, (uint32_t)s32[1]));
}

// Online softmax of one query block over one key tile, offset-in-accumulator form, log2 domain.  The S^T accumulators were STARTED at -m_run
// (the column's reference offset) and q carries ch^-1/2 log2(e), so they hold s - m_run and p = exp2(sacc): max, exp2, add per element and
// no multiply.  The offset moves only when the tile's maximum exceeds it by more than 8 (p <= 2^8); then the tile is shifted and O / l are
// rescaled on a wave-uniform slow path.  `first` (the column's first key tile) always takes that path: its offset becomes the tile maximum,
// whatever its sign.  On return sacc holds P^T and l_run the lane's share of the row sums (attn_store_normalised reduces it).
template <int MT, int CI>
__device__ __forceinline__ void attn_softmax_offset(f32x4 (&sacc)[MT], f32x4 (&o)[CI], float& m_run, float& l_run, bool first) {
  float mx = fmaxf(fmaxf(sacc[0][0], sacc[0][1]), fmaxf(sacc[0][2], sacc[0][3]));
#pragma unroll
  for (int mi = 1; mi < MT; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sacc[mi][r]);
  mx = attn_colmax(mx);
  const float delta = first ? mx : (mx > 8.0f ? mx : 0.0f);
  if (first || __builtin_amdgcn_ballot_w64(delta != 0.0f) != 0) {   // wave-uniform: some column's offset moves
    const float alpha = first ? 1.0f : __builtin_amdgcn_exp2f(-delta);
    m_run += delta;
    l_run *= alpha;
#pragma unroll
    for (int mi = 0; mi < MT; ++mi)
#pragma unroll
      for (int r = 0; r < 4; ++r) sacc[mi][r] -= delta;
#pragma unroll
    for (int ci = 0; ci < CI; ++ci)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[ci][r] *= alpha;
  }
  float psum = 0.f;
#pragma unroll
  for (int mi = 0; mi < MT; ++mi)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float pv = __builtin_amdgcn_exp2f(sacc[mi][r]);
      sacc[mi][r] = pv;
      psum += pv;
    }
  l_run += psum;
}

// o[qb][ci] += tile^T (channels 16 ci .. + 15 as MFMA rows) x sacc[qb] (its 16 MT rows are the summed index): O^T += V^T P^T of the forward,
// dQ^T += K^T dS^T, dV^T += dA^T P and dK^T += Q^T dS of the backward.  A tile fragment is read once and used by all QB column blocks.
template <typename T, int ROW, int MT, int CI, int QB>
__device__ __forceinline__ void attn_pv(f32x4 (&o)[QB][CI], const f32x4 (&sacc)[QB][MT], const char* tile, int lr, int lq) {
  constexpr int FT = attn_frag_tiles<T>();
#pragma unroll
  for (int s2 = 0; s2 < MT / FT; ++s2) {
    u32x4 pfrag[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) pfrag[qb] = attn_acc_frag<T>(sacc[qb][FT * s2], sacc[qb][FT * s2 + FT - 1]);
#pragma unroll
    for (int ci = 0; ci < CI; ++ci) {
      const u32x4 vf = attn_tr_frag<T, ROW>(tile, 16 * FT * s2, ci, lr, lq);
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) mma16(o[qb][ci], vf, pfrag[qb], T());
    }
  }
}

// CI accumulator tiles of one column -> its row of an NHWC tensor: the lane holds channels 16 ci + 4 lq + r, scaled by `scale` (1.0f: as they
// are).  The caller guards the column.
template <typename T, int CI>
__device__ __forceinline__ void attn_store_quads(T* row, const f32x4 (&o)[CI], float scale, int lq) {
#pragma unroll
  for (int ci = 0; ci < CI; ++ci) {
    const f32x4 v = f32x4{o[ci][0] * scale, o[ci][1] * scale, o[ci][2] * scale, o[ci][3] * scale};
    if constexpr (Elem<T>::DTYPE == 1) *reinterpret_cast<u32x2*>(row + ci * 16 + 4 * lq) = pack4(v, T());
    else *reinterpret_cast<f32x4*>(row + ci * 16 + 4 * lq) = v;
  }
}
// the forward's last step: l summed over the four lanes of the column, O / l stored.  Every lane calls it (the shuffles stay outside the
// guard, as the kernels had them); `live` = the column is inside the tensor (q < T), `row` is not touched otherwise.
template <typename T, int CI>
__device__ __forceinline__ void attn_store_normalised(T* row, bool live, const f32x4 (&o)[CI], float l, int lq) {
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  const float inv = 1.0f / l;
  if (live) attn_store_quads<T, CI>(row, o, inv, lq);
}

// Row-major staging of ROWS rows of two tensors (K | V, or Q | dA) into two LDS tiles of the layout above, by 256 threads: thread
// `tid` owns the 16-byte fragments e = tid + 256 u (row e / FPR, slot e % FPR) of both; tensor row r starts at base + r * stride (elements),
// rows from `nrows` on are zero.  Two halves, global -> registers and registers -> LDS, so that a caller can keep the loads in flight over a
// tile's MFMAs.
template <typename T, int CH, int ROWS> constexpr int attn_stage_frags() { return (ROWS * (CH / Elem<T>::VEC) + 255) / 256; }
template <typename T, int CH, int ROWS, int NF>
__device__ __forceinline__ void attn_stage_rows_load(u32x4 (&a)[NF], u32x4 (&b)[NF], const T* abase, size_t astride, const T* bbase, size_t bstride,
                                                     int row0, int nrows, int tid) {
  constexpr int V = Elem<T>::VEC, FPR = CH / V;
  static_assert(NF == attn_stage_frags<T, CH, ROWS>(), "fragments per thread");
#pragma unroll
  for (int u = 0; u < NF; ++u) {
    const int e = tid + 256 * u, s = e / FPR, f = e - s * FPR;
    const int row = row0 + s;
    a[u] = u32x4{0u, 0u, 0u, 0u}; b[u] = u32x4{0u, 0u, 0u, 0u};
    if (e < ROWS * FPR && row < nrows) {
      a[u] = *reinterpret_cast<const u32x4*>(abase + (size_t)row * astride + f * V);
      b[u] = *reinterpret_cast<const u32x4*>(bbase + (size_t)row * bstride + f * V);
    }
  }
}
template <typename T, int CH, int ROWS, int NF>
__device__ __forceinline__ void attn_stage_rows_store(char* atile, char* btile, const u32x4 (&a)[NF], const u32x4 (&b)[NF], int tid) {
  constexpr int FPR = CH / Elem<T>::VEC, ROW = CH * (int)sizeof(T) + 32;
#pragma unroll
  for (int u = 0; u < NF; ++u) {
    const int e = tid + 256 * u, s = e / FPR, f = e - s * FPR;
    if (e < ROWS * FPR) {
      *reinterpret_cast<u32x4*>(atile + s * ROW + f * 16) = a[u];
      *reinterpret_cast<u32x4*>(btile + s * ROW + f * 16) = b[u];
    }
  }
}
