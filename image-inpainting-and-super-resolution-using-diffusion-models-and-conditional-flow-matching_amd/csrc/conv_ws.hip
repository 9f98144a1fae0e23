// The warp-specialised persistent 3x3 conv as a unit of its own: the kernel and its launcher (conv_ws.inc.h) and the family's route / launch (ops.h).
#include "conv_kargs.h"
#include "conv_epilogue.h"

namespace {
#include "conv_ws.inc.h"
}  // namespace

// Shapes the warp-specialised kernel takes (everything else stays on the plain kernel): the plain tile choice already was the
// largest one (>= 512 workgroups of 128 x 128), 3x3 / stride 1 / NHWC output, an even number of 64-byte channel chunks
// (row pairs and chunk pairs are unrolled), images of at least one 16 x 16 tile, and at least one tile per CU.
// ... and may carry the ResBlock's 1x1 skip conv (knob bit 1): a GroupNorm prologue form without split weights, plain geometry, no residual of its
// own, whole 64-byte skip chunks
int ws_route(const ConvDesc& d, const ConvPre& p, ConvRoute* r) {
  const Geo& g = p.g;
  const ConvKArgs& a = p.a;
  const int enabled = p.K->conv_ws;
  if (!(enabled & 1) || d.ks != 3 || g.BM != 128 || g.BN != 128 || g.G != 1 || g.bn_pack != 128 || d.out_mode != OUT_NHWC) return 1;
  if (g.stride != 1 || a.nchunks < 2 || (a.nchunks & 1)) return 1;
  if (g.Wo < ws::VW || g.Ho < ws::TH) return 1;
  const int tiles = ((g.Wo + ws::VW - 1) / ws::VW) * ((g.Ho + ws::TH - 1) / ws::TH);   // 16 x 16 pixel tiles per image
  const int n_mt = d.N * tiles, n_nt = (d.Cout + 127) / 128;
  if (!(enabled & 4) && n_mt * n_nt < ws_num_cus()) return 1;   // fewer tiles than CUs: the plain kernel's smaller tiles fill the chip better (knob bit 2, tests: take them too)
  if (p.fskip) {
    const int CH = d.dtype == 0 ? 16 : 32;
    if (!(enabled & 2) || !a.pro_a || d.wsplit || d.mode != CONV_UNIT || d.act_out || a.res_mode != RES_NONE) return 1;
    if (a.SC0 <= 0 || a.SC0 % CH || a.SC1 % CH) return 1;
  }
  r->kernel = CONV_K_WS; r->skip = p.fskip ? 1 : 0;
  r->geom.BM = 256; r->geom.lds_bytes = ws::LDS_BYTES;
  const int slots = 2 * tiles;   // (16x16 pixel tile, 8-row half) per image
  if (p.gn_ok && slots <= d.gn_slots_cap) r->gn_slots = slots;
  return 0;
}

int ws_launch(const ConvDesc& d, const ConvPre& p, const ConvRoute&, hipStream_t stream) {
  return dispatch_dtype(d.dtype, [&](auto t) { return launch_ws<decltype(t)>(p.a, p.K->conv_ws >> 8, stream); });
}
