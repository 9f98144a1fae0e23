// Vector-Jacobian product of the U-Net w.r.t. its image input: the plan of unet_engine.hip walked in reverse.
//
// Reference: the reconstruction-guidance sampler differentiates the x0 model through the network,
// `vmap(grad(constraint, argnums=0))(xi, i, condition)` (AD/image_diffusion/sampling.py:154-163); every sample's loss depends on
// its own image only (GroupNorm and attention are per sample), so vmap(grad) over the batch IS one batched backward pass.
// Only data gradients exist here (no weight gradients: inference), so each forward op has a short adjoint:
//   conv (+ residual, + emb)     residual: grad[res] += G (or its 2x2 block sums for the nearest-x2 residual of ResBlock(up));
//                                data: the same implicit-GEMM kernels on transposed / tap-flipped weights (conv_pack_weights_dgrad);
//                                stride 2: zero-stuff G first; nearest-x2 input: 2x2 block sums of the result;
//                                two sources (skip concat): one conv, the halves of its output go to the two gradients
//   GroupNorm32 (+SiLU, +FiLM)   gn_silu_bwd (backward.hip) from the site's kept (a, b, mean, rstd)
//   attention core               attention_bwd (attention_bwd.hip) from the kept qkv tensor
//   avg-pool / nearest-up        gathers (backward.hip)
// Every activation of the forward is still in the workspace (the plan never reuses an arena slot); gradients live in a second arena
// of the same layout and are written by their first contributor, added to by the others.
#include "unet_engine.h"

// The conv branch's data gradient (ops.h ConvDgradDesc): the walker below and the test op mi355_conv2d_vjp run this one sequence.
namespace {
// the bias-free NHWC unit-mode conv of the (zero-stuffed) output gradient with the transposed filter
ConvDesc dgrad_conv(const ConvDgradDesc& d) {
  ConvDesc c; c.dtype = d.dtype; c.N = d.N; c.ks = d.ks; c.mode = CONV_UNIT; c.knobs = d.knobs; c.err = d.err;
  c.w = d.wT; c.Cout = d.cin_pad; c.out = d.du; c.out_mode = OUT_NHWC; c.C0 = d.Cg;
  if (d.mode == CONV_STRIDE2) { c.src0 = d.zbuf; c.Hs = d.Hs; c.Ws = d.Ws; }   // at the input resolution
  else { c.src0 = d.G; c.Hs = d.Hg; c.Ws = d.Wg; }
  return c;
}
}  // namespace

int conv_dgrad_route(const ConvDgradDesc& d, ConvRoute* r) { return conv_route(dgrad_conv(d), r); }

int conv_dgrad_launch(const ConvDgradDesc& d, hipStream_t stream, ConvDgradOut* out) {
  MI355_REQUIRE(out && d.G && d.wT && d.du, -1, "conv dgrad: null argument");
  MI355_REQUIRE(d.mode == CONV_UNIT || d.mode == CONV_STRIDE2 || d.mode == CONV_UP2, -4, "conv dgrad: the forward conv's mode must be unit, stride 2 or nearest x2");
  MI355_REQUIRE(d.mode != CONV_STRIDE2 || d.zbuf, -1, "conv dgrad: a stride-2 conv needs the zero-stuffing scratch");
  MI355_REQUIRE(d.scatter ? d.g0 != nullptr : (d.mode != CONV_UP2 || d.tmp), -1, "conv dgrad: no destination");
  int rc;
  // stride 2: zero insertion back to the input resolution, then a stride-1 conv with the flipped taps
  if (d.mode == CONV_STRIDE2 && (rc = grad_gather_launch(d.dtype, d.zbuf, d.G, d.N, d.Hs, d.Ws, d.Cg, d.Hg, d.Wg, d.Cg, 0, GATHER_STUFF, 0, 1.0f, stream))) return rc;
  const ConvDesc c = dgrad_conv(d);
  const int Hd = c.Hs, Wd = c.Ws;   // resolution of the data-gradient conv's output
  if ((rc = conv_route(c, &out->route))) return rc;
  if ((rc = conv_launch(c, out->route, stream))) return rc;
  // nearest-x2 input (Upsample / ResBlock(up)): the conv saw up2(u), so du(u) = 2x2 block sums of the conv's data gradient
  const bool up = d.mode == CONV_UP2;
  out->dU = d.du; out->dU_stride = d.cin_pad;
  if (!d.scatter) {
    if (up) {
      if ((rc = grad_gather_launch(d.dtype, d.tmp, d.du, d.N, d.Hs, d.Ws, d.cin_pad, Hd, Wd, d.cin_pad, 0, GATHER_POOL, 0, 1.0f, stream))) return rc;
      out->dU = d.tmp;
    }
    return 0;
  }
  const int mode = up ? GATHER_POOL : GATHER_SAME;
  if ((rc = grad_gather_launch(d.dtype, d.g0, d.du, d.N, d.Hs, d.Ws, d.C0, Hd, Wd, d.cin_pad, 0, mode, d.acc0, 1.0f, stream))) return rc;
  if (d.g1 && (rc = grad_gather_launch(d.dtype, d.g1, d.du, d.N, d.Hs, d.Ws, d.C1, Hd, Wd, d.cin_pad, d.C0, mode, d.acc1, 1.0f, stream))) return rc;
  return 0;
}

int unet_backward(const mi355_unet* net, const float* grad_out, float* grad_x, int Cx, int B, void* workspace, int64_t workspace_bytes,
                  hipStream_t stream) {
  MI355_REQUIRE(net && grad_out && grad_x && workspace, -1, "unet_vjp: null argument");
  MI355_REQUIRE(net->cfg.differentiable, -4, "unet_vjp: the handle was not created with cfg.differentiable = 1");
  MI355_REQUIRE(B > 0 && Cx > 0 && Cx <= net->cfg.in_channels, -2, "unet_vjp: bad batch / channel count");
  const WsView v(net, workspace, B);
  MI355_REQUIRE((int64_t)v.l.total <= workspace_bytes, -2, "unet_vjp: workspace too small");
  const int dtype = net->cfg.dtype, CH = dtype == 0 ? 16 : 32;
  const char* W = net->dev_weights;
  void* du = v.at(v.l.du); void* tmp = v.at(v.l.tmp); void* zbuf = v.at(v.l.z); void* dyp = v.at(v.l.dy);
  std::vector<char> written(net->tensors.size(), 0);
  int rc;
  auto site = [&](int k, GnBwdDesc& g) { const WsView::Site s = v.site(k); g.a = s.a; g.b = s.b; g.mean = s.mean; g.rstd = s.rstd; };
  // grad[id] (+)= gather(src)
  auto accumulate = [&](int id, const void* src, int Hs, int Ws, int cs, int coff, int mode, float scale) -> int {
    const PlanTensor& t = net->tensors[id];
    const int r = grad_gather_launch(dtype, v.grad(id), src, B, t.H, t.W, t.C, Hs, Ws, cs, coff, mode, written[id], scale, stream);
    written[id] = 1;
    return r;
  };
  const int S = net->cfg.image_size;
  for (int oi = (int)net->ops.size() - 1; oi >= 0; --oi) {
    const PlanOp& op = net->ops[oi];
    const PlanTensor& s0 = net->tensors[op.src0];
    const int C1 = op.src1 >= 0 ? net->tensors[op.src1].C : 0;
    if (op.kind == OP_GN) continue;   // folded into its consumer's adjoint
    if (op.kind == OP_CONV) {
      // ---- G = gradient of the conv's output ----
      const void* G; int Hg, Wg, Cg;
      if (op.dst < 0) {   // network output (NCHW fp32): pack the caller's cotangent, channel-padded to one chunk
        if ((rc = pack_nhwc_launch(dtype, grad_out, op.Cout, nullptr, 0, B, S * S, CH, dyp, stream))) return rc;
        G = dyp; Hg = S; Wg = S; Cg = CH;
      } else {
        MI355_REQUIRE(written[op.dst], -4, "unet_vjp: a conv output has no gradient (plan order)");
        const PlanTensor& d = net->tensors[op.dst];
        G = v.grad(op.dst); Hg = d.H; Wg = d.W; Cg = d.C;
      }
      // ---- residual operand ----
      if (op.res >= 0) {
        if (op.res_mode == RES_SAME) rc = accumulate(op.res, G, Hg, Wg, Cg, 0, GATHER_SAME, 1.0f);
        else rc = accumulate(op.res, G, Hg, Wg, Cg, 0, GATHER_POOL, 1.0f);   // forward added nearest-x2(res): sum the 2x2 blocks
        if (rc) return rc;
      }
      // ---- data gradient through the conv (conv_dgrad_launch below): scattered to the sources, or left for the GroupNorm adjoint ----
      ConvDgradDesc c; c.dtype = dtype; c.G = G; c.Cg = Cg; c.Hg = Hg; c.Wg = Wg;
      c.wT = W + op.wT_off; c.cin_pad = op.cin_pad; c.ks = op.ks; c.mode = op.mode;
      c.N = B; c.Hs = s0.H; c.Ws = s0.W; c.du = du; c.tmp = tmp; c.zbuf = zbuf;
      c.scatter = !op.use_pro;
      if (c.scatter) {
        c.g0 = v.grad(op.src0); c.C0 = s0.C; c.acc0 = written[op.src0];
        if (op.src1 >= 0) { c.g1 = v.grad(op.src1); c.C1 = C1; c.acc1 = written[op.src1]; }
      }
      ConvDgradOut o;
      if ((rc = conv_dgrad_launch(c, stream, &o))) return rc;
      if (op.use_pro) {
        GnBwdDesc g; g.dtype = dtype; g.x0 = v.tensor(op.src0); g.C0 = s0.C; g.x1 = op.src1 >= 0 ? v.tensor(op.src1) : nullptr; g.C1 = C1;
        g.du = o.dU; g.du_stride = o.dU_stride; g.N = B; g.HW = s0.H * s0.W; g.silu = op.pro_silu;
        site(op.gn_site, g);
        g.g0 = v.grad(op.src0); g.acc0 = written[op.src0];
        if (op.src1 >= 0) { g.g1 = v.grad(op.src1); g.acc1 = written[op.src1]; }
        if ((rc = gn_silu_bwd_launch(g, stream))) return rc;
      }
      written[op.src0] = 1;
      if (op.src1 >= 0) written[op.src1] = 1;
    } else if (op.kind == OP_ATTN) {
      MI355_REQUIRE(written[op.dst], -4, "unet_vjp: an attention output has no gradient (plan order)");
      AttnBwdDesc a; a.dtype = dtype; a.qkv = v.tensor(op.src0); a.a = v.tensor(op.dst); a.da = v.grad(op.dst); a.dqkv = v.grad(op.src0);
      a.N = B; a.T = s0.H * s0.W; a.heads = op.heads; a.ch = op.ch; a.new_order = net->cfg.use_new_attention_order;
      a.L = v.f32(v.l.ld); a.D = a.L + (size_t)B * op.heads * a.T;
      if ((rc = attention_bwd_launch(a, stream))) return rc;
      written[op.src0] = 1;   // q, k and v parts are all written: the qkv tensor has this one consumer
    } else if (op.kind == OP_POOLAFF) {
      // forward: out = avgpool2(silu(a x + b)): each input position got 1/4 of its block's gradient
      MI355_REQUIRE(written[op.dst], -4, "unet_vjp: a pooled tensor has no gradient (plan order)");
      const PlanTensor& d = net->tensors[op.dst];
      if ((rc = grad_gather_launch(dtype, tmp, v.grad(op.dst), B, s0.H, s0.W, s0.C, d.H, d.W, d.C, 0, GATHER_UP, 0, 0.25f, stream))) return rc;
      GnBwdDesc g; g.dtype = dtype; g.x0 = v.tensor(op.src0); g.C0 = s0.C; g.du = tmp; g.du_stride = s0.C; g.N = B; g.HW = s0.H * s0.W;
      g.silu = op.pro_silu;
      site(op.gn_site, g);
      g.g0 = v.grad(op.src0); g.acc0 = written[op.src0];
      if ((rc = gn_silu_bwd_launch(g, stream))) return rc;
      written[op.src0] = 1;
    } else if (op.kind == OP_RESAMPLE) {
      MI355_REQUIRE(written[op.dst], -4, "unet_vjp: a resampled tensor has no gradient (plan order)");
      const PlanTensor& d = net->tensors[op.dst];
      if (op.mode == CONV_POOL2) rc = accumulate(op.src0, v.grad(op.dst), d.H, d.W, d.C, 0, GATHER_UP, 0.25f);
      else rc = accumulate(op.src0, v.grad(op.dst), d.H, d.W, d.C, 0, GATHER_POOL, 1.0f);
      if (rc) return rc;
    } else {
      mi355_set_error("unet_vjp: op kind without an adjoint in a differentiable plan");
      return -4;
    }
  }
  MI355_REQUIRE(written[net->in_tensor], -4, "unet_vjp: the input received no gradient");
  return unpack_channels_launch(dtype, v.grad(net->in_tensor), B, S * S, net->in_pad, 0, Cx, grad_x, stream);
}
