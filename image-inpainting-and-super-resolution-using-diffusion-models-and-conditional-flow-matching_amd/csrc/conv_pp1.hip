// The ping-pong 1x1 conv as a unit of its own: the kernel (conv_pp1.inc.h, on the wait / barrier helpers of conv_pp.inc.h, whose kernel is not instantiated
// here) and the family's route / launch (ops.h).
#include "conv_kargs.h"
#include "conv_epilogue.h"

namespace {
#include "conv_pp.inc.h"
#include "conv_pp1.inc.h"
}  // namespace

// 0 = taken, 1 = not this kernel (the stationary-tile / generic kernels), < 0 = error.  mode: mi355_debug_config::conv_pp.  (Hi / lo split
// weights never come here: conv_route sends them to the generic kernels.)
int pp1_route(const ConvDesc& d, ConvRoute* r) {
  const mi355_debug_config& K = d.knobs ? *d.knobs : mi355_default_debug();
  const int CH = d.dtype == 0 ? 16 : 32, esz = d.dtype == 0 ? 4 : 2;
  if (!K.conv_pp || d.ks != 1 || d.mode != CONV_UNIT || d.out_mode != OUT_NHWC || d.pro_a) return 1;
  if (d.Cout % 128 != 0 || d.C0 % CH != 0 || d.C1 % CH != 0 || conv_tile_n(d.Cout) != 128) return 1;
  const int wide = d.Cout % 256 == 0;
  const int HW = d.Hs * d.Ws;
  // half-height wide tiles (conv_pp bit 5) where the wide walk would give a CU fewer than two tiles
  const bool half = wide && (K.conv_pp & 32) && HW % 256 == 0 && (long)d.N * HW / 256 * (d.Cout / 256) < 2L * ws_num_cus();
  const int BM = half ? 128 : (wide ? 256 : 512), BN = wide ? 256 : 128;
  const int Cin = d.C0 + d.C1, nchunks = Cin / CH;
  // (four chunks: the old stationary-tile kernel ties - 128 -> 256 at 16x16: 13.4 vs 13.9 us - and stays)
  if (nchunks < 8 || (nchunks & 3) || (HW % BM) != 0) return 1;
  if (d.res && d.res_mode != RES_SAME) return 1;
  const int n_mt = (int)((long)d.N * HW / BM), n_nt = d.Cout / BN;
  if ((K.conv_pp & 3) < 2 && n_mt * n_nt < ws_num_cus()) return 1;
  const size_t b0 = (size_t)d.N * HW * d.C0 * esz, b1 = (size_t)d.N * HW * d.C1 * esz, ob = (size_t)d.N * HW * d.Cout * esz;
  const size_t wb = conv_packed_weight_bytes(d.dtype, d.Cout, Cin, 1);
  MI355_REQUIRE(b0 < 0xFFFF0000ull && b1 < 0xFFFF0000ull && wb < 0xFFFF0000ull && ob < 0xFFFF0000ull, -4,
                "conv1x1: a tensor exceeds 4 GiB (32-bit buffer offsets): run the batch in slices");
  r->kernel = CONV_K_1X1_PP; r->form = half ? 2 : wide; r->n_mt = n_mt; r->n_nt = n_nt;
  const int slots = HW / (half ? 64 : 128);   // (pixel tile of the image, a wave's pixel part)
  r->gn_slots = d.gn_stats && slots <= d.gn_slots_cap ? slots : 0;
  return 0;
}

int pp1_launch(const ConvDesc& d, const ConvRoute& r, hipStream_t stream) {
  const mi355_debug_config& K = d.knobs ? *d.knobs : mi355_default_debug();
  const int CH = d.dtype == 0 ? 16 : 32, esz = d.dtype == 0 ? 4 : 2;
  const int Cin = d.C0 + d.C1, HW = d.Hs * d.Ws;
  ConvKArgs a{};
  a.src0 = d.src0; a.src1 = d.src1; a.C0 = d.C0; a.C1 = d.C1; a.Cin = Cin; a.nchunks = a.nreal = Cin / CH;
  a.N = d.N; a.Hs = d.Hs; a.Ws = d.Ws; a.Hc = d.Hs; a.Wc = d.Ws; a.Ho = d.Hs; a.Wo = d.Ws;
  a.w = d.w; a.bias = d.bias; a.Cout = d.Cout; a.bn_pack = 128;
  a.emb = d.emb; a.emb_stride = d.emb_stride;
  a.res = d.res; a.res_mode = d.res ? RES_SAME : RES_NONE; a.Hr = d.Hs; a.Wr = d.Ws;
  a.out = d.out; a.out_mode = OUT_NHWC;
  a.bytes0 = (uint32_t)((size_t)d.N * HW * d.C0 * esz); a.bytes1 = d.src1 ? (uint32_t)((size_t)d.N * HW * d.C1 * esz) : 0u;
  a.wbytes = (uint32_t)conv_packed_weight_bytes(d.dtype, d.Cout, Cin, 1); a.obytes = (uint32_t)((size_t)d.N * HW * d.Cout * esz); a.rbytes = d.res ? a.obytes : 0u;
  a.ablate = K.conv_ablate; a.err = d.err; a.spin_limit = 1;
  if (r.gn_slots) { a.gn_stats = d.gn_stats; a.gn_slots = r.gn_slots; }
  const int rc = dispatch_dtype(d.dtype, [&](auto t) {
    using T = decltype(t);
    return r.form == 2 ? pp1_launch_k<T, 2>(a, r.n_mt, r.n_nt, stream) : (r.form ? pp1_launch_k<T, 1>(a, r.n_mt, r.n_nt, stream) : pp1_launch_k<T, 0>(a, r.n_mt, r.n_nt, stream));
  });
  if (rc) return rc;
  MI355_CHECK_HIP(hipGetLastError());
  return 0;
}
