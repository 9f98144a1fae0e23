// What the MFMA conv kernels share behind their multiplication (conv_igemm.hip, conv_ws.hip, conv_pp.hip, conv_pp1.hip, conv_small.hip, conv1x1.hip,
// conv_edge.hip): the pieces of the store epilogue, the persistent kernels' tile walk and the ping-pong kernels' accumulator start values.
//
// Epilogue layout of every kernel here: MFMA rows are channels and columns are pixels, so lane (lr, lq) holds, per 16 x 16 tile (mi, ni), the 4
// consecutive channels 16 ni + 4 lq .. + 3 of pixel lr.  fp32 stores that quad as it is (16 bytes).  The 16-bit types merge the quads of a PAIR of channel
// tiles (2 k, 2 k + 1) into one 16-byte store by two v_permlane16_swap: lane (lr, lq) then holds the 8 channels 32 k + 16 (lq & 1) + 8 (lq >> 1) .. + 7
// of pixel lr (the callers' co_s), and a residual piece loaded at the same address comes back to the accumulator layout by the same two swaps.
//
// What is NOT here, and why: the row loop of the three persistent kernels (residual loads, residual add, GnPartial::add, stores) stays written out in
// the kernels.  conv_ws.inc.h and conv_pp.inc.h write it on epi_pair_unswap / epi_pair_store.  conv_pp1.inc.h uses NOTHING of this header in its kernel
// (only persistent_grid in its launcher): conv1x1_pp_kernel keeps its own walk lambdas, start values and pair epilogue, because on the shared forms it
// spilled more and its launches ran 1-2 % slower.  So a change to TileWalk, the start values or the pair primitives has a second home there.
// GnPartial::add's first call of a tile sums two products (hi * hi + lo * lo), and the compiler contracts one of them into the FMA; with the loop, or
// only the residual add of a pair, inside a helper it contracts the OTHER one in those kernels and their 16-bit outputs change in the last bit
// (profiles/conv_epilogue_parity.md lists the forms tried).
// The invariant is: these kernels' outputs equal, bit for bit, what they were before this header existed; a change here is checked against that.
#pragma once
#include "conv_kargs.h"

namespace {

// ---- pair primitives (16-bit element types) ----
// un-swap an 8-channel residual piece back to the accumulator layout: ra / rb = the lane's quads of channel tiles 2 k / 2 k + 1
template <typename T>
__device__ __forceinline__ void epi_pair_unswap(const u32x4& r, float (&ra)[4], float (&rb)[4], T) {
  const auto s0 = __builtin_amdgcn_permlane16_swap(r[0], r[2], false, false);
  const auto s1 = __builtin_amdgcn_permlane16_swap(r[1], r[3], false, false);
  const uint32_t xa[2] = {s0[0], s1[0]}, xb[2] = {s0[1], s1[1]};
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    unpack2(xa[q], ra[2 * q], ra[2 * q + 1], T());
    unpack2(xb[q], rb[2 * q], rb[2 * q + 1], T());
  }
}
// the 16 bytes lane (lr, lq) stores for the quads va / vb (float[4] or f32x4) of a pair of channel tiles
template <typename V, typename T>
__device__ __forceinline__ u32x4 epi_pair_pack(const V& va, const V& vb, T) {
  const u32x2 pa2 = pack4(va, T()), pb2 = pack4(vb, T());
  const auto w0 = __builtin_amdgcn_permlane16_swap(pa2[0], pb2[0], false, false);
  const auto w1 = __builtin_amdgcn_permlane16_swap(pa2[1], pb2[1], false, false);
  return u32x4{w0[0], w1[0], w0[1], w1[1]};
}
template <typename V, typename T>
__device__ __forceinline__ void epi_pair_store(const V& va, const V& vb, __amdgpu_buffer_rsrc_t rs, uint32_t byte_offset, T) {
  __builtin_amdgcn_raw_buffer_store_b128(epi_pair_pack(va, vb, T()), rs, byte_offset, 0, 0);
}

// ---- quad primitives (fp32) ----
template <bool HAS_RES>
__device__ __forceinline__ f32x4 epi_quad_res(f32x4 o, const u32x4& res_piece) {
  if constexpr (HAS_RES) {
    const f32x4 t = __builtin_bit_cast(f32x4, res_piece);
    o = f32x4{o[0] + t[0], o[1] + t[1], o[2] + t[2], o[3] + t[3]};
  }
  return o;
}
__device__ __forceinline__ void epi_quad_store(const f32x4& o, __amdgpu_buffer_rsrc_t rs, uint32_t byte_offset) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, o), rs, byte_offset, 0, 0);
}

// ---- the persistent kernels' tile walk (conv3x3_ws_kernel, conv3x3_pp_kernel; conv1x1_pp_kernel has the same walk as lambdas of its own) ----
// Items t = 0 .. ntp - 1: 8 consecutive workgroups (one per XCD) take 8 consecutive pixel tiles, the workgroup 8 further on (same XCD, same L2) the
// next channel tile of the same pixels.  The pixel tiles are padded to a multiple of 8, so an item may be no tile (mt >= n_mt): next_valid skips it.
struct TileWalk {
  int n_mt, n_nt, ntp, nwg, wg;
  __device__ __forceinline__ TileWalk(int n_mt_, int n_nt_, int nwg_, int wg_) : n_mt(n_mt_), n_nt(n_nt_), ntp(((n_mt_ + 7) / 8) * 8 * n_nt_), nwg(nwg_), wg(wg_) {}
  __device__ __forceinline__ void decode(int t, int& mt, int& nt) const {
    const int per = 8 * n_nt, blk = t / per, r = t - blk * per;
    nt = r >> 3; mt = blk * 8 + (r & 7);
  }
  __device__ __forceinline__ int next_valid(int t) const {   // next item of this workgroup's walk that is a real tile (or >= ntp)
    for (t += nwg; t < ntp; t += nwg) { int mt, nt; decode(t, mt, nt); if (mt < n_mt) break; }
    return t;
  }
  __device__ __forceinline__ int first() const { return next_valid(wg - nwg); }   // >= ntp: this workgroup has no tile
};

// ---- accumulator start values of the ping-pong 3x3 kernel (conv1x1_pp_kernel has the same text of its own) ----
// bias (+ the embedding row of image n0) of the lane's channels co .. co + 3, co = nt * BN + wn * 64 + 16 ni + 4 lq (Cout % BN == 0: always in range):
// loaded while the previous tile is stored; the accumulators of all MI pixel tiles start from them.
__device__ __forceinline__ f32x4 epi_cinit_quad(const ConvKArgs& p, int co, int n0) {
  f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
  if (p.bias) v = *reinterpret_cast<const f32x4*>(p.bias + co);
  if (p.emb) { const f32x4 e = *reinterpret_cast<const f32x4*>(p.emb + (size_t)n0 * p.emb_stride + co); v = f32x4{v[0] + e[0], v[1] + e[1], v[2] + e[2], v[3] + e[3]}; }
  return v;
}
template <int MI, int NI>
__device__ __forceinline__ void epi_acc_init(f32x4 (&acc)[MI][NI], const f32x4 (&cin)[NI]) {
#pragma unroll
  for (int mi = 0; mi < MI; ++mi)
#pragma unroll
    for (int ni = 0; ni < NI; ++ni) acc[mi][ni] = cin[ni];
}

}  // namespace
