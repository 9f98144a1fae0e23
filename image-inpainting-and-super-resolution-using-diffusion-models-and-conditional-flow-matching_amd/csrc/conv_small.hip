// The 8x8 / 4x4-level 3x3 conv as a unit of its own: the kernel and its launcher (conv_small.inc.h) and the family's route / launch (ops.h).
#include <algorithm>
#include <cstring>

#include "conv_kargs.h"
#include "conv_epilogue.h"

namespace {
#include "conv_small.inc.h"
}  // namespace

// Shapes this kernel takes: 3x3, whole 8x8 / 4x4 OUTPUT images, stride 1 (plain or nearest-x2 input) or - round 5 - stride 2 (the Downsample convs
// 16 -> 8 and 8 -> 4, AD/image_diffusion/unet.py:217-240: the staged patch is the (2 Ho + 1)^2 input window, the fragment addresses step two
// pixels per output pixel: 2-way bank conflicts on reads that are a tenth of this kernel's LDS budget), no GroupNorm prologue (these
// levels normalise in a pass of their own), NHWC output with C_out % 128 == 0, residual at the output resolution or none.
// 0 = taken (r: ksplit, waves, w8x2, sm::Args, LDS, fused skip conv, the GroupNorm sites applied), 1 = not this kernel (the plain kernel), < 0 = error.
int small_route(const ConvDesc& d, const ConvPre& p, ConvRoute* r) {
  const ConvKArgs& a = p.a;
  const int enabled = p.K->conv_small;
  const bool act = d.act_out && (p.K->gn_epilogue & 1) && d.act_out != d.out, act2 = act && d.act2_out && (p.K->gn_epilogue & 4);
  const size_t esz = d.dtype == 0 ? 4 : 2;
  MI355_REQUIRE(!act || (size_t)d.N * a.Ho * a.Wo * (d.act_stride ? d.act_stride : d.Cout) * esz < 0xFFFF0000ull, -4,
                "conv: activated output exceeds 4 GiB (32-bit buffer offsets): run the batch in slices");
  MI355_REQUIRE(!act2 || (size_t)d.N * a.Ho * a.Wo * (d.act2_stride ? d.act2_stride : d.Cout) * esz < 0xFFFF0000ull, -4,
                "conv: activated output exceeds 4 GiB (32-bit buffer offsets): run the batch in slices");
  if (!enabled || d.ks != 3 || a.out_mode != OUT_NHWC || a.pro_a) return 1;
  const bool s2 = a.stride == 2;
  const bool skip = a.sk0 != nullptr;
  if (skip && (!(enabled & 8) || s2 || a.mode != CONV_UNIT || a.res_mode != RES_NONE || a.src1 || a.nchunks != a.nreal)) return 1;
  if (s2 && (!(enabled & 4) || a.mode != CONV_STRIDE2 || a.Hc != 2 * a.Ho || a.Wc != 2 * a.Wo)) return 1;
  if (a.Ho != a.Wo || (a.Ho != 8 && a.Ho != 4) || a.Cout % 128 != 0) return 1;
  if (a.res_mode != RES_NONE && a.res_mode != RES_SAME) return 1;
  const int CH = d.dtype == 0 ? 16 : 32;
  if (a.C0 % CH || a.C1 % CH) return 1;
  const bool w8 = a.Ho == 8;
  sm::Args g;
  const int G = w8 ? 1 : 4, PW = s2 ? 2 * a.Ho + 1 : a.Ho + 2;
  g.pwp = s2 ? PW : (w8 ? 16 : 8); g.sh = w8 ? 1 : 2;
  g.pimg = PW * g.pwp;
  g.plane = (G * g.pimg - (g.pwp - PW)) * 64;
  const int nchp = s2 ? (w8 ? 8 : 4) : (w8 ? 16 : 8);
  g.nphase = (a.nchunks + nchp - 1) / nchp;
  g.chp = a.nchunks / g.nphase;
  if (g.chp * g.nphase != a.nchunks) return 1;
  const int tiles = (a.N + G - 1) / G;
  // waves along N: as many as keep every CU busy (each halving doubles the workgroups and splits K between wave pairs)
  const int ncu = ws_num_cus();
  int nw = 4;
  while (nw > 1 && (long)tiles * (a.Cout / (64 * nw)) < ncu) nw >>= 1;
  if (a.Cout % (64 * nw)) return 1;
  const int ksplit = 4 / nw;
  if (g.chp % ksplit) return 1;
  g.red_bytes = ksplit > 1 ? 4 * 16 * 1024 : 0;
  g.sphase = g.schp = g.sup = 0;
  if (skip) {
    if (a.SC0 % CH || a.SC1 % CH) return 1;
    const int ns = (a.SC0 + a.SC1) / CH;
    g.sup = g.nphase == 1 && ns <= sm::SDMAX && ns % ksplit == 0 && (size_t)g.chp * g.plane + (size_t)ns * sm::SPLANE <= 160 * 1024;
    g.sphase = g.sup ? 1 : (ns + nchp - 1) / nchp;
    g.schp = ns / g.sphase;
    if (g.schp * g.sphase != ns || g.schp % ksplit) return 1;
  }
  const size_t lds = g.sup ? std::max((size_t)g.chp * g.plane + (size_t)g.schp * sm::SPLANE, (size_t)g.red_bytes)
                           : std::max((size_t)std::max(g.chp, g.schp) * g.plane, (size_t)g.red_bytes);
  if (lds > 160 * 1024) return 1;
  r->kernel = CONV_K_SMALL; r->ksplit = ksplit; r->n_mt = tiles; r->n_nt = a.Cout / (64 * nw); r->lds = lds; r->skip = skip;
  // whole-chip launches of the 8x8 level (one image per workgroup, no K split): eight waves of 32 channels (knob conv_small bit 1)
  r->form = w8 && !s2 && !skip && ksplit == 1 && (enabled & 2) && a.Cout % 256 == 0;
  static_assert(sizeof(r->sm) == sizeof(sm::Args), "ConvRoute::sm holds sm::Args");
  memcpy(r->sm, &g, sizeof g);
  // GroupNorm of the output in the epilogue: whole images per wave (an 8x8 image split over K-sharing waves is not), 4 / 8 / 16 channels per group
  auto cpg_ok = [&](int cpg, int coff) { return (cpg == 4 || cpg == 8 || cpg == 16) && d.Cout % cpg == 0 && coff % cpg == 0; };
  const bool ok = act && cpg_ok(d.act_cpg ? d.act_cpg : d.Cout / 32, d.act_coff) && (a.Ho != 8 || r->ksplit == 1);
  const bool ok2 = ok && act2 && cpg_ok(d.act2_cpg ? d.act2_cpg : d.Cout / 32, d.act2_coff);
  r->act_done = (ok ? 1 : 0) | (ok2 ? 2 : 0);
  return 0;
}

// the GroupNorm sites the route applies (ConvRoute::act_done; conv_launch has copied the first one's act_out .. act_raw), then the kernel
int small_launch(const ConvDesc& d, const ConvPre& p, const ConvRoute& r, hipStream_t stream) {
  ConvKArgs a = p.a;
  const size_t esz = d.dtype == 0 ? 4 : 2;
  if (r.act_done & 1) {
    a.act_stride = d.act_stride ? d.act_stride : d.Cout; a.act_coff = d.act_coff; a.act_cpg = d.act_cpg ? d.act_cpg : d.Cout / 32;
    a.abytes = (uint32_t)((size_t)d.N * a.Ho * a.Wo * a.act_stride * esz);
    a.warm = (p.K->l2_warm & 1) ? d.warm : nullptr; a.warm_bytes = a.warm ? d.warm_bytes : 0u;
  }
  if (r.act_done & 2) {
    a.act2_out = d.act2_out; a.act2_gamma = d.act2_gamma; a.act2_beta = d.act2_beta; a.act2_silu = d.act2_silu;
    a.act2_stride = d.act2_stride ? d.act2_stride : d.Cout; a.act2_coff = d.act2_coff; a.act2_cpg = d.act2_cpg ? d.act2_cpg : d.Cout / 32;
    a.a2bytes = (uint32_t)((size_t)d.N * a.Ho * a.Wo * a.act2_stride * esz);
  }
  return dispatch_dtype(d.dtype, [&](auto t) { return launch_small<decltype(t)>(a, r, stream); });
}
