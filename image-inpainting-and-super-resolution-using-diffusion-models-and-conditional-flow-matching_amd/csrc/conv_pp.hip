// The ping-pong persistent 3x3 conv as a unit of its own: the kernel and its launchers (conv_pp.inc.h) and the family's route / launch (ops.h).
#include "conv_kargs.h"
#include "conv_epilogue.h"

#ifndef PP_IMPL   // experiments: make variant VARFLAGS='-DPP_IMPL="\"../../tools/experiments/<file>\""' VARTAG=_x builds a library around another version of the kernel
#define PP_IMPL "conv_pp.inc.h"
#endif
namespace {
#include PP_IMPL
}  // namespace

// Shapes the ping-pong kernel takes: 3x3 / stride 1 / NHWC output, input either as it is or through the GroupNorm affine + SiLU prologue
// (PRO = 2; an affine-only prologue stays on the other kernels), an even number of 64-byte channel chunks per source switch (two chunks
// are unrolled; a source boundary may fall anywhere), images of at least one tile.  Geometry: Cout % 256 == 0 -> wide (16 x 16 x 256);
// otherwise Cout % 128 == 0 and Wo >= 32 -> narrow (16 x 32 x 128).  mode = mi355_debug_config::conv_pp: bits 0-1: 1 = only when every CU
// gets a tile, 2 = always (tests); bit 2: the prologue form of the wide geometry; bit 3: the narrow geometry; bit 4: the prologue form of the
// narrow geometry too (off by default: same-box it ties the warp-specialised kernel at 256 / 384 input channels and loses 3-5 % at 128,
// profiles/r5_experiments.md - the prologue's arithmetic is amortised over 128 output channels instead of 256).
// Bit 6 (64): the phase form of a prologue-free conv over a nearest-x2 up-sampled input (four 2x2 convs of the low-res image, UP = 1: 4/9 of
// the MFMAs): wide geometry only, the geometry rule and the tile count apply to the LOW-RES image (16 x 16 low-res pixels per tile, four phase
// tiles each); it needs the collapsed weight image and carries no residual, split weights or fused output norm.
// ConvRoute::form is the geometry (0 wide, 1 narrow, 2 wide in phase form).  A fused skip conv is not looked at: the kernel does not carry one (conv_route).
int pp_route(const ConvDesc& d, const ConvPre& p, ConvRoute* r) {
  const Geo& g = p.g;
  const ConvKArgs& a = p.a;
  const int mode = p.K->conv_pp, Ho = g.Ho, Wo = g.Wo, Cout = d.Cout;
  if (!(mode & 3) || d.ks != 3 || g.G != 1 || g.bn_pack != 128 || d.out_mode != OUT_NHWC || g.stride != 1) return 1;
  if (p.has_pro && !d.pro_silu) return 1;
  if (a.nchunks < 2 || (a.nchunks & 1)) return 1;
  const bool up_ok = d.mode == CONV_UP2 && d.w_up2 && !d.wsplit && a.res_mode == RES_NONE;
  if (up_ok && (mode & 64) && !p.has_pro && Cout % 256 == 0 && !(Ho & 1) && !(Wo & 1) && Ho >= 32 && Wo >= 32) {
    const int tiles = ((d.Ws + 15) / 16) * ((d.Hs + 15) / 16);   // low-res pixel tiles per image
    if ((mode & 3) >= 2 || 4 * d.N * tiles * (Cout / 256) >= ws_num_cus()) {
      r->kernel = CONV_K_PP; r->form = 2; r->w_up2 = 1;
      r->geom.BM = 256; r->geom.BN = 256; r->geom.lds_bytes = pp::D<0>::lds_bytes(false);
      const int slots = 4 * 2 * tiles;   // (phase, low-res pixel tile, pixel wave) per image
      if (p.gn_ok && slots <= d.gn_slots_cap) r->gn_slots = slots;
      return 0;
    }
  }
  int cfg = -1;
  if (Cout % 256 == 0 && Wo >= 16 && Ho >= 16) cfg = 0;
  else if (Cout % 128 == 0 && (mode & 8) && Wo >= 32 && Ho >= 16) cfg = 1;
  if (cfg < 0) return 1;
  if (p.has_pro && !(mode & (cfg == 0 ? 4 : 16))) return 1;
  const int vw = cfg == 0 ? 16 : 32, bn = cfg == 0 ? 256 : 128;
  const int tiles = ((Wo + vw - 1) / vw) * ((Ho + 15) / 16);   // pixel tiles per image
  if ((mode & 3) < 2 && d.N * tiles * (Cout / bn) < ws_num_cus()) return 1;
  r->kernel = CONV_K_PP; r->form = cfg;
  r->geom.BM = cfg == 0 ? 256 : 512; r->geom.BN = bn;
  r->geom.lds_bytes = cfg == 0 ? pp::D<0>::lds_bytes(p.has_pro) : pp::D<1>::lds_bytes(p.has_pro);
  // the output GroupNorm in place (the activated tensor replaces the raw one): one 16 x 16 tile per image, no residual, 8 or 16 channels per group
  const bool act = cfg == 0 && Ho == 16 && Wo == 16 && (Cout == 256 || Cout == 512) && a.res_mode == RES_NONE;
  if (act && d.act_out && (p.K->gn_epilogue & 2) && d.act_out == d.out && !d.act_raw) r->act_done = 1;
  const int slots = (cfg == 0 ? 2 : 4) * tiles;   // (pixel tile, pixel wave) per image
  if (!r->act_done && p.gn_ok && slots <= d.gn_slots_cap) r->gn_slots = slots;
  return 0;
}

int pp_launch(const ConvDesc& d, const ConvPre& p, const ConvRoute& r, hipStream_t stream) {
  ConvKArgs a = p.a;
  if (r.w_up2) {
    MI355_REQUIRE(d.w_up2, -1, "conv: the route asks for the collapsed up-sampling weights (conv_pack_weights_up2) and the description has none");
    a.w = d.w_up2; a.wbytes = (uint32_t)conv_packed_weight_bytes_up2(d.dtype, d.Cout, d.C0 + d.C1);
  }
  return dispatch_dtype(d.dtype, [&](auto t) { return launch_pp<decltype(t)>(a, r.form, stream); });
}
