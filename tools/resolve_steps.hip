// Host-only check of the forward resolver (csrc/unet_engine.hip: unet_resolve): plans a U-Net without parameters or weights, resolves one
// forward against made-up pointers and prints one line per step.  Nothing is launched and no device is needed; build it with the host code
// under a sanitizer (make -C <package>/csrc resolve_steps) and run it: it must exit 0 with no report.  The launched steps plus the prelude
// of each listing are the launch count mi355_unet_get_stats reports for the same forward on a GPU (tools/sampler_digest.py, fwd_* cases).
#include <cstdio>
#include <cstring>

#include "../image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd/csrc/unet_engine.h"

namespace {

mi355_unet_config cifar(int film) {
  mi355_unet_config c{};
  c.image_size = 32; c.in_channels = 3; c.model_channels = 128; c.out_channels = 3; c.num_res_blocks = 2;
  c.n_attention_ds = 1; c.attention_ds[0] = 2;
  c.n_channel_mult = 4; const int m[4] = {1, 2, 2, 2}; memcpy(c.channel_mult, m, sizeof m);
  c.conv_resample = 1; c.num_heads = 4; c.num_head_channels = 64; c.num_heads_upsample = -1;
  c.use_scale_shift_norm = film; c.dtype = MI355_BF16;
  return c;
}
mi355_unet_config flowers64() {
  mi355_unet_config c = cifar(1);
  c.image_size = 64; c.in_channels = 6; c.num_res_blocks = 1; c.attention_ds[0] = 4;
  const int m[4] = {1, 2, 3, 4}; memcpy(c.channel_mult, m, sizeof m);
  c.resblock_updown = 1;
  return c;
}

const char* kernel_name(int k) {
  static const char* n[] = {"igemm", "1x1", "1x1_pp", "in", "out", "pp", "ws", "small"};
  return k >= 0 && k < 8 ? n[k] : "?";
}

struct Line {
  const mi355_unet* net; size_t i;
  void head(const char* what) const {
    const PlanOp& op = net->ops[i];
    const PlanTensor& s = net->tensors[op.src0];
    printf("  %3zu %-14s src %3d,%3d -> %3d  %4dx%-3d C %4d", i, what, op.src0, op.src1, op.dst, s.H, s.W, s.C + (op.src1 >= 0 ? net->tensors[op.src1].C : 0));
  }
  void operator()(const GnAbsorbed&) const { head("gn:absorbed"); printf("\n"); }
  void operator()(const GnFinDesc& g) const { head("gn:finalize"); printf("  slots %d,%d film %d\n", g.slots0, g.slots1, g.film != nullptr); }
  void operator()(const GnDesc& g) const { head(g.y ? "gn:apply" : "gn:stats"); printf("  film %d silu %d site %d\n", g.film != nullptr, g.y_silu, g.mean != nullptr); }
  void operator()(const ConvCarried&) const { head("conv:carried"); printf("\n"); }
  void operator()(const ConvStep& c) const {
    head("conv");
    const ConvDesc& d = c.c; const ConvRoute& r = c.rt;
    printf("  ks %d mode %d Cout %4d  %-6s form %d tile %dx%d  pro %d emb %d res %d  act asked %d%d done %d raw %d inplace %d  gn_slots %d skip %d nchw %d axpy %d up2 %d\n",
           d.ks, d.mode, d.Cout, kernel_name(r.kernel), r.form, r.geom.BM, r.geom.BN, d.pro_a != nullptr, d.emb != nullptr, d.res_mode,
           d.act_out != nullptr, d.act2_out != nullptr, r.act_done, d.act_raw, d.act_out && d.act_out == d.out, r.gn_slots, r.skip, r.reads_nchw, r.axpy, r.w_up2);
  }
  void operator()(const AttnDesc& a) const { head("attention"); printf("  heads %d ch %d T %d\n", a.heads, a.ch, a.T); }
  void operator()(const AttnFusedDesc& a) const { head("attn:fused"); printf("  heads %d ch %d T %d\n", a.heads, a.ch, a.T); }
  void operator()(const PoolAffStep& p) const { head("pool+affine"); printf("  silu %d\n", p.silu); }
  void operator()(const ResampleStep& r) const { head("resample"); printf("  mode %d\n", r.mode); }
};

int run(const char* name, const mi355_unet_config& cfg, int B) {
  mi355_unet net;
  const int64_t wbytes = unet_plan_dry(cfg, &net);
  if (wbytes < 0) { fprintf(stderr, "%s: plan failed: %s\n", name, mi355_last_error()); return 1; }
  // made-up addresses (never dereferenced): weights, a 256-byte-aligned workspace, the caller's tensors
  net.dev_weights = reinterpret_cast<char*>(uintptr_t(1) << 40);
  void* ws = reinterpret_cast<void*>(uintptr_t(2) << 40);
  float* x = reinterpret_cast<float*>(uintptr_t(3) << 40);
  float* out = reinterpret_cast<float*>(uintptr_t(4) << 40);
  const float* cond = cfg.in_channels > 3 ? reinterpret_cast<const float*>(uintptr_t(5) << 40) : nullptr;
  ResolvedForward f;
  const int rc = unet_resolve(WsView(&net, ws, B), x, 3, cond, cfg.in_channels - 3, out, UnetRun(), &f);
  if (rc) { fprintf(stderr, "%s B=%d: resolve failed (%d): %s\n", name, B, rc, mi355_last_error()); return 1; }
  int64_t launched = 0;
  for (const ForwardStep& s : f.steps) launched += unet_step_launches(s);
  printf("%s B=%d: %zu plan ops, weight image %lld bytes, workspace %lld bytes\n", name, B, net.ops.size(), (long long)wbytes,
         (long long)unet_workspace_bytes(&net, B));
  printf("  prelude: embedding path %d, pack_nhwc %d\n", f.emb, (int)f.pack);
  for (size_t i = 0; i < f.steps.size(); ++i) std::visit(Line{&net, i}, f.steps[i]);
  printf("  launched steps %lld + prelude %lld = %lld launches\n", (long long)launched, (long long)(unet_launch_count(f) - launched), (long long)unet_launch_count(f));
  return 0;
}

}  // namespace

int main() {
  int bad = 0;
  for (int B : {8, 256}) {
    bad += run("cifar", cifar(0), B);
    bad += run("cifar_film", cifar(1), B);
    bad += run("flowers64_updown", flowers64(), B);
  }
  return bad ? 1 : 0;
}
