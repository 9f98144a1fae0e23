// U-Net layer plan, weight packer and executor.
//
// Rebuilds the wiring of UNetModel.__init__/forward (AD/image_diffusion/unet.py:521-728; identical to
// torchcfm's UNetModelWrapper used by cifar10/ and mnist/) as a flat list of fused device ops:
//   ResBlock  (unet.py:331-351) = GN-stats, conv3x3[GN+SiLU prologue, +emb epilogue], GN-stats(+FiLM),
//                                  (1x1 skip conv), conv3x3[GN+SiLU prologue, +skip epilogue]
//   Attention (unet.py:395-401) = GN-stats, 1x1 conv[GN prologue] -> qkv, fused attention, 1x1 conv[+x]
//   Down/Upsample, skip concat, nearest-up / avg-pool are gather modes of the consuming conv.
// Parameters arrive in the reference's state_dict order and layouts and are repacked once.
#include "unet_engine.h"

#include <algorithm>
#include <cstring>
#include <map>

namespace {

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// The blocks of UNetModel.__init__ (unet.py:564-706) in construction order = state_dict order.  The input_blocks.N / output_blocks.N.j numbering,
// the attention test and the stack of skip channel counts live here and nowhere else: unet_enumerate_params names the parameters of this
// list, Walker::walk plans its ops.
enum BlockKind { BLK_CONV_IN, BLK_RES, BLK_ATTN, BLK_RESAMPLE_CONV, BLK_RESAMPLE, BLK_OUT };
struct Block {
  std::string prefix;   // of its state_dict entries (BLK_RESAMPLE has none; BLK_OUT: "out", i.e. out.0 and out.2)
  int kind, cin, cout;  // cin of a popping ResBlock counts the skip's channels too (unet.py:650); BLK_OUT: cin = the first conv's output channels
  int dir = 0;          // BLK_RES: ResBlock(up) > 0, ResBlock(down) < 0; BLK_RESAMPLE_CONV: Upsample.conv > 0, Downsample.op < 0; BLK_RESAMPLE likewise
  bool upsample = false;   // BLK_ATTN on the up path (num_heads_upsample, unet.py:370-378)
  bool push = false, pop = false;   // its output goes onto the skip stack / its input is cat([h, hs.pop()])
};
std::vector<Block> unet_blocks(const mi355_unet_config& cfg) {
  const int mc = cfg.model_channels, nl = cfg.n_channel_mult;
  auto has_attn = [&](int ds) { for (int i = 0; i < cfg.n_attention_ds; ++i) if (cfg.attention_ds[i] == ds) return true; return false; };
  std::vector<Block> out;
  auto add = [&](const std::string& prefix, int kind, int cin, int cout, int dir = 0) -> Block& {
    Block b; b.prefix = prefix; b.kind = kind; b.cin = cin; b.cout = cout; b.dir = dir;
    out.push_back(b);
    return out.back();
  };
  // a level change: ResBlock(up/down), Downsample.op / Upsample.conv, or the plain pool / nearest-x2 (which has no parameters)
  auto resample = [&](const std::string& p, const char* conv_name, int ch, int dir) -> Block& {
    if (cfg.resblock_updown) return add(p, BLK_RES, ch, ch, dir);
    if (cfg.conv_resample) return add(p + conv_name, BLK_RESAMPLE_CONV, ch, ch, dir);
    return add(p, BLK_RESAMPLE, ch, ch, dir);
  };
  int ch = cfg.channel_mult[0] * mc;
  const int input_ch = ch;
  add("input_blocks.0.0", BLK_CONV_IN, cfg.in_channels, ch).push = true;
  std::vector<int> chans{ch};
  int ds = 1, idx = 1;
  for (int level = 0; level < nl; ++level) {
    const int mult = cfg.channel_mult[level];
    for (int r = 0; r < cfg.num_res_blocks; ++r, ++idx) {
      const std::string p = "input_blocks." + std::to_string(idx);
      add(p + ".0", BLK_RES, ch, mult * mc);
      ch = mult * mc;
      if (has_attn(ds)) add(p + ".1", BLK_ATTN, ch, ch);
      out.back().push = true;
      chans.push_back(ch);
    }
    if (level != nl - 1) {
      resample("input_blocks." + std::to_string(idx) + ".0", ".op", ch, -1).push = true;
      chans.push_back(ch);
      ds *= 2; ++idx;
    }
  }
  add("middle_block.0", BLK_RES, ch, ch); add("middle_block.1", BLK_ATTN, ch, ch); add("middle_block.2", BLK_RES, ch, ch);
  idx = 0;
  for (int level = nl - 1; level >= 0; --level) {
    const int mult = cfg.channel_mult[level];
    for (int i = 0; i <= cfg.num_res_blocks; ++i, ++idx) {
      const std::string p = "output_blocks." + std::to_string(idx);
      const int ich = chans.back(); chans.pop_back();
      add(p + ".0", BLK_RES, ch + ich, mc * mult).pop = true;
      ch = mc * mult;
      int j = 1;
      if (has_attn(ds)) { add(p + "." + std::to_string(j), BLK_ATTN, ch, ch).upsample = true; ++j; }
      if (level && i == cfg.num_res_blocks) {
        resample(p + "." + std::to_string(j), ".conv", ch, +1);
        ds /= 2;
      }
    }
  }
  add("out", BLK_OUT, input_ch, cfg.out_channels);
  return out;
}

struct Walker {
  mi355_unet_config cfg;
  int dtype, esz, CH;
  bool dry;
  const float* const* host = nullptr;
  std::vector<ParamInfo> params;
  std::map<std::string, int> pidx;
  std::vector<char> blob;
  size_t cursor = 0;
  mi355_unet* net = nullptr;
  std::string err;
  struct EmbPart { std::string name; int off, width; };
  std::vector<EmbPart> emb_parts;
  int emb_total = 0;
  int last_site = -1;   // differentiable plans: the GroupNorm site the next prologue consumer applies

  int heads_for(int ch, bool upsample) const {  // unet.py:370-378
    if (cfg.num_head_channels == -1) {
      int nh = (upsample && cfg.num_heads_upsample != -1) ? cfg.num_heads_upsample : cfg.num_heads;
      return nh;
    }
    return ch / cfg.num_head_channels;
  }

  size_t alloc(size_t bytes) {
    size_t o = cursor;
    cursor = align_up(cursor + bytes, 256);
    if (!dry) blob.resize(cursor, 0);
    return o;
  }
  const float* P(const std::string& name, std::vector<int64_t> expect) {
    auto it = pidx.find(name);
    if (it == pidx.end()) { err = "missing parameter " + name; return nullptr; }
    if (params[it->second].shape != expect) { err = "shape mismatch for " + name; return nullptr; }
    return dry ? nullptr : host[it->second];
  }
  size_t put_f32(const std::string& name, std::vector<int64_t> shape) {
    const float* p = P(name, shape);
    int64_t n = 1; for (auto s : shape) n *= s;
    size_t o = alloc((size_t)n * 4);
    if (!dry && p) memcpy(blob.data() + o, p, (size_t)n * 4);
    return o;
  }
  size_t put_conv(const std::string& name, int Cout, int Cin, int ks, bool conv1d) {
    std::vector<int64_t> shape = conv1d ? std::vector<int64_t>{Cout, Cin, 1} : std::vector<int64_t>{Cout, Cin, ks, ks};
    const float* p = P(name, shape);
    size_t bytes = conv_packed_weight_bytes(dtype, Cout, Cin, ks, net->wsplit);
    size_t o = alloc(bytes);
    if (!dry && p) conv_pack_weights(dtype, p, Cout, Cin, ks, blob.data() + o, net->wsplit);
    net->weight_bytes += (double)Cout * Cin * ks * ks * esz;
    return o;
  }
  size_t put_linear_t(const std::string& name, int J, int K) {  // W [J][K] -> Wt [K][J]
    const float* p = P(name, {J, K});
    size_t o = alloc((size_t)J * K * 4);
    if (!dry && p) {
      float* d = reinterpret_cast<float*>(blob.data() + o);
      for (int j = 0; j < J; ++j) for (int k = 0; k < K; ++k) d[(size_t)k * J + j] = p[(size_t)j * K + k];
    }
    return o;
  }

  int tensor(int C, int H, int W) {
    PlanTensor t{C, H, W, false, net->act_elems_per_image};
    net->act_elems_per_image += align_up((size_t)C * H * W, 128);
    net->tensors.push_back(t);
    return (int)net->tensors.size() - 1;
  }
  const PlanTensor& T(int id) const { return net->tensors[id]; }

  // Returns -1 (the consumer conv applies a*x + b (+SiLU) in its staging prologue) or, for small images, the id of a tensor
  // that already holds silu?(GN(x)): at 8x8 and below the convs are latency-bound 64-pixel-tile launches whose prologue math
  // and per-image (a, b) loads sit on the critical path, while the GN kernel has the whole image in L2 anyway.
  int add_gn(int s0, int s1, const std::string& wname, const std::string& bname, int film_off, int apply_silu, bool may_apply = true) {
    const int max_hw = net->knobs.gn_apply_max_hw;
    const int C = T(s0).C + (s1 >= 0 ? T(s1).C : 0);
    PlanOp op; op.kind = OP_GN; op.src0 = s0; op.src1 = s1;
    op.gamma_off = put_f32(wname, {C}); op.beta_off = put_f32(bname, {C}); op.film_emb_off = film_off;
    if (cfg.differentiable) {
      // the backward pass re-derives everything from (x, a, b, mean, rstd) of each site: no applied copies, no shared (a, b) buffer
      op.gn_site = last_site = (int)net->site_C.size();
      net->site_C.push_back(C);
      net->site_off.push_back(net->site_floats_per_image);
      net->site_floats_per_image += (size_t)2 * C + 64;
    } else if (may_apply && T(s0).H * T(s0).W <= max_hw) { op.dst = tensor(C, T(s0).H, T(s0).W); op.pro_silu = apply_silu; }
    else {
      // larger images: take the statistics from the partial sums the producing convs leave in their epilogues when the groups are
      // whole channel quads of each source (C multiple of 128 for GroupNorm32); decided per launch (a producer that cannot
      // provide them, e.g. a resample pass, leaves the site on the statistics kernel)
      const int fuse = net->knobs.gn_fuse;
      const int C1 = s1 >= 0 ? T(s1).C : 0;
      if (fuse && (C / 32) % 4 == 0 && T(s0).C % 4 == 0 && C1 % 4 == 0) {
        op.fin_ok = 1;
        for (int s : {s0, s1}) {
          if (s < 0 || net->tensors[s].stats_cap) continue;
          PlanTensor& t = net->tensors[s];
          t.stats_cap = gn_stats_cap(t.H * t.W);
          t.stats_off_per_image = net->stats_floats_per_image;
          net->stats_floats_per_image += (size_t)t.stats_cap * (t.C / 4) * 2;
        }
      }
    }
    net->ops.push_back(op);
    if (C > net->max_gn_c) net->max_gn_c = C;
    return op.dst;
  }
  // returns dst tensor (or -1 for the NCHW fp32 network output)
  int add_conv(const std::string& prefix, int s0, int s1, int Cin_logical, int Cout, int ks, int mode, bool conv1d, int use_pro,
               int pro_silu, int emb_off, int res, int res_mode, int out_mode) {
    PlanOp op; op.kind = OP_CONV; op.src0 = s0; op.src1 = s1; op.mode = mode; op.ks = ks; op.Cout = Cout;
    op.w_off = put_conv(prefix + ".weight", Cout, Cin_logical, ks, conv1d);
    op.bias_off = put_f32(prefix + ".bias", {Cout});
    op.use_pro = use_pro; op.pro_silu = pro_silu; op.emb_off = emb_off; op.res = res; op.res_mode = res_mode; op.out_mode = out_mode;
    // Upsample.conv in a shape the phase form of the ping-pong kernel could take (conv_pp bit 6; the route looks at batch and knobs again per launch)
    const int cin_t = T(s0).C + (s1 >= 0 ? T(s1).C : 0);
    if (mode == CONV_UP2 && ks == 3 && !conv1d && !use_pro && res < 0 && out_mode == OUT_NHWC && !cfg.differentiable && !net->wsplit && (net->knobs.conv_pp & 64) &&
        Cout % 256 == 0 && cin_t == Cin_logical && T(s0).H >= 16 && T(s0).W >= 16) {
      const float* pw = P(prefix + ".weight", {Cout, Cin_logical, ks, ks});
      op.has_wu = 1; op.wu_off = alloc(conv_packed_weight_bytes_up2(dtype, Cout, Cin_logical));
      if (!dry && pw) conv_pack_weights_up2(dtype, pw, Cout, Cin_logical, blob.data() + op.wu_off);
    }
    int Ho = T(s0).H, Wo = T(s0).W;
    if (mode == CONV_UP2) { Ho *= 2; Wo *= 2; }
    else if (mode == CONV_POOL2) { Ho /= 2; Wo /= 2; }
    else if (mode == CONV_STRIDE2) { Ho = (Ho - 1) / 2 + 1; Wo = (Wo - 1) / 2 + 1; }
    op.dst = out_mode == OUT_NHWC ? tensor(Cout, Ho, Wo) : -1;
    if (cfg.differentiable) {
      if (use_pro) op.gn_site = last_site;
      op.cin_pad = conv_dgrad_cin_pad(T(s0).C, s1 >= 0 ? T(s1).C : 0);
      const float* pw = P(prefix + ".weight", conv1d ? std::vector<int64_t>{Cout, Cin_logical, 1} : std::vector<int64_t>{Cout, Cin_logical, ks, ks});
      op.wT_off = alloc(conv_packed_weight_bytes_dgrad(dtype, Cout, Cin_logical, ks, op.cin_pad));
      if (!dry && pw) conv_pack_weights_dgrad(dtype, pw, Cout, Cin_logical, ks, op.cin_pad, blob.data() + op.wT_off);
      // scratch of the backward pass: the data-gradient conv's output (at the conv's own input resolution, before any pooling back),
      // the zero-stuffed output gradient of a stride-2 conv, the pooled gradient of an up-sampling conv with a prologue
      const size_t hw_dgrad = mode == CONV_UP2 ? (size_t)Ho * Wo : (size_t)T(s0).H * T(s0).W;
      net->bwd_du_elems = std::max(net->bwd_du_elems, hw_dgrad * op.cin_pad);
      if (mode == CONV_STRIDE2) net->bwd_z_elems = std::max(net->bwd_z_elems, (size_t)T(s0).H * T(s0).W * Cout);
      net->bwd_tmp_elems = std::max(net->bwd_tmp_elems, (size_t)T(s0).H * T(s0).W * op.cin_pad);
    }
    net->ops.push_back(op);
    const double in_elems = (double)(T(s0).C + (s1 >= 0 ? T(s1).C : 0)) * T(s0).H * T(s0).W;
    net->conv_flops += 2.0 * Ho * Wo * (double)Cout * Cin_logical * ks * ks;
    net->act_bytes += (in_elems + (double)Cout * Ho * Wo) * esz;
    return op.dst;
  }

  int res_block(const std::string& p, int s0, int s1, int cin, int cout, bool up, bool down) {
    const bool film = cfg.use_scale_shift_norm != 0;
    const int ew = film ? 2 * cout : cout;
    const int eoff = emb_total;
    emb_parts.push_back({p + ".emb_layers.1", eoff, ew});
    emb_total += ew;
    P(p + ".emb_layers.1.weight", {ew, 4 * cfg.model_channels});
    P(p + ".emb_layers.1.bias", {ew});
    const int y1 = add_gn(s0, s1, p + ".in_layers.0.weight", p + ".in_layers.0.bias", -1, 1, !down);
    int h1;
    int res = s0, res_mode = up ? RES_UP2 : RES_SAME;
    if (down) {
      // ResBlock(down=True): h = conv(AvgPool(SiLU(GN(x)))), x -> AvgPool(x) (unet.py:332-337): both pools are small HBM-bound
      // pre-passes (the first one fused with the GN affine + SiLU), so the conv itself stays a plain stride-1 conv.
      if (s1 >= 0) { err = "ResBlock(down) over a channel concat is not supported"; return -1; }
      PlanOp op; op.kind = OP_POOLAFF; op.src0 = s0; op.pro_silu = 1;
      op.dst = tensor(T(s0).C, T(s0).H / 2, T(s0).W / 2);
      if (cfg.differentiable) { op.gn_site = last_site; net->bwd_tmp_elems = std::max(net->bwd_tmp_elems, (size_t)T(s0).H * T(s0).W * T(s0).C); }
      net->ops.push_back(op);
      h1 = add_conv(p + ".in_layers.2", op.dst, -1, cin, cout, 3, CONV_UNIT, false, 0, 0, film ? -1 : eoff, -1, RES_NONE, OUT_NHWC);
      res = resample(s0, CONV_POOL2);
    } else {
      h1 = y1 >= 0 ? add_conv(p + ".in_layers.2", y1, -1, cin, cout, 3, up ? CONV_UP2 : CONV_UNIT, false, 0, 0, film ? -1 : eoff, -1, RES_NONE, OUT_NHWC)
                   : add_conv(p + ".in_layers.2", s0, s1, cin, cout, 3, up ? CONV_UP2 : CONV_UNIT, false, 1, 1, film ? -1 : eoff, -1, RES_NONE, OUT_NHWC);
    }
    const int y2 = add_gn(h1, -1, p + ".out_layers.0.weight", p + ".out_layers.0.bias", film ? eoff : -1, 1);
    if (cin != cout) {
      if (up || down) { err = "ResBlock(up/down) with a channel change is not supported"; return -1; }
      auto it = pidx.find(p + ".skip_connection.weight");
      const int sks = (it != pidx.end() && params[it->second].shape.size() == 4) ? (int)params[it->second].shape[3] : 1;
      res = add_conv(p + ".skip_connection", s0, s1, cin, cout, sks, CONV_UNIT, false, 0, 0, -1, -1, RES_NONE, OUT_NHWC);
      res_mode = RES_SAME;
    } else if (s1 >= 0) {
      err = "identity skip over a channel concat is not supported";
      return -1;
    }
    const int skip_idx = cin != cout ? (int)net->ops.size() - 1 : -1;
    // The 1x1 skip_connection can ride in the second conv as centre-tap K chunks of the raw block input (unet.py:312-317, 351: return
    // skip_connection(x) + h), if the launch agrees (conv_route).  Small levels (apply-type norms: the second conv reads one already-activated
    // tensor): the small-level kernel, conv_small bit 3.  Levels at least 16 pixels wide (the second conv carries the GroupNorm + SiLU prologue):
    // the warp-specialised kernel, conv_ws bit 1.  Both weight images are kept: a launch that declines runs the two convs on their own.
    auto carry_skip = [&](int out) {
      if (out < 0 || skip_idx < 0 || net->ops[skip_idx].ks != 1 || cfg.differentiable || net->wsplit || cout % 128 != 0) return;
      const int conv2_idx = (int)net->ops.size() - 1;
      PlanOp& c2 = net->ops[conv2_idx];
      const float* w3 = P(p + ".out_layers.3.weight", {cout, cout, 3, 3});
      const float* w1 = P(p + ".skip_connection.weight", {cout, cin, 1, 1});
      const float* b3 = P(p + ".out_layers.3.bias", {cout});
      const float* b1 = P(p + ".skip_connection.bias", {cout});
      c2.wf_off = alloc(conv_packed_weight_bytes_skip(dtype, cout, cout, cin));
      c2.bf_off = alloc((size_t)cout * 4);
      if (!dry && w3 && w1 && b3 && b1) {
        conv_pack_weights_skip(dtype, w3, w1, cout, cout, cin, blob.data() + c2.wf_off);
        float* bs = reinterpret_cast<float*>(blob.data() + c2.bf_off);
        for (int i = 0; i < cout; ++i) bs[i] = b3[i] + b1[i];
      }
      c2.skip_op = skip_idx;
      net->ops[skip_idx].carrier = conv2_idx;
    };
    if (y2 >= 0) {
      const int out = add_conv(p + ".out_layers.3", y2, -1, cout, cout, 3, CONV_UNIT, false, 0, 0, -1, res, res_mode, OUT_NHWC);
      carry_skip(out);
      return out;
    }
    const int out = add_conv(p + ".out_layers.3", h1, -1, cout, cout, 3, CONV_UNIT, false, 1, 1, -1, res, res_mode, OUT_NHWC);
    // (Cout % 256 != 0: what the warp-specialised kernel takes in the network; the 256-channel 16x16 blocks run on the ping-pong kernel, whose
    //  route declines the fused form - no second weight image and no probe for them)
    if (out >= 0 && T(h1).W >= 16 && T(h1).H >= 16 && cout % 256 != 0) carry_skip(out);
    return out;
  }

  int attn_block(const std::string& p, int x, int C, int heads) {
    if (heads <= 0 || C % heads != 0) { err = "attention: bad head count"; return -1; }
    const int ch = C / heads;
    {
      bool ok = false;
      for (int v : {32, 64, 96, 128, 192, 256, 384, 512}) ok = ok || ch == v;
      if (!ok) { err = "attention: head channels must be one of 32, 64, 96, 128, 192, 256, 384, 512 (got " + std::to_string(ch) + ")"; return -1; }
    }
    if (cfg.differentiable && ch > 256) {   // attention_bwd.hip instantiates head sizes up to 256: fail at build, not in the middle of a guidance loop
      err = "attention: differentiable plans support head channels up to 256 (got " + std::to_string(ch) + ")";
      return -1;
    }
    const int yn = add_gn(x, -1, p + ".norm.weight", p + ".norm.bias", -1, 0);
    const double Tn_ = (double)T(x).H * T(x).W;
    if (yn < 0 && !cfg.differentiable && !net->wsplit && attn_fused_eligible(dtype, T(x).H * T(x).W, C, heads, ch, &net->knobs)) {
      // norm-apply + qkv 1x1 + attention in one kernel (attn_fused.hip): the [T, 3C] qkv tensor never exists
      PlanOp op; op.kind = OP_ATTN_FUSED; op.src0 = x; op.heads = heads; op.ch = ch; op.Cout = 3 * C;
      op.w_off = put_conv(p + ".qkv.weight", 3 * C, C, 1, true);
      op.bias_off = put_f32(p + ".qkv.bias", {3 * C});
      op.dst = tensor(C, T(x).H, T(x).W);
      net->ops.push_back(op);
      net->conv_flops += 2.0 * Tn_ * 3.0 * C * C;
      net->attn_flops += 4.0 * Tn_ * Tn_ * C;
      net->act_bytes += (2.0 * C * Tn_) * esz;   // x in, attention output out: the qkv tensor is not algorithmic traffic any more
      return add_conv(p + ".proj_out", op.dst, -1, C, C, 1, CONV_UNIT, true, 0, 0, -1, x, RES_SAME, OUT_NHWC);
    }
    const int qkv = yn >= 0 ? add_conv(p + ".qkv", yn, -1, C, 3 * C, 1, CONV_UNIT, true, 0, 0, -1, -1, RES_NONE, OUT_NHWC)
                            : add_conv(p + ".qkv", x, -1, C, 3 * C, 1, CONV_UNIT, true, 1, 0, -1, -1, RES_NONE, OUT_NHWC);
    PlanOp op; op.kind = OP_ATTN; op.src0 = qkv; op.heads = heads; op.ch = ch;
    op.dst = tensor(C, T(x).H, T(x).W);
    net->ops.push_back(op);
    if (cfg.differentiable) net->bwd_ld_floats = std::max(net->bwd_ld_floats, (size_t)2 * heads * T(x).H * T(x).W);
    const double Tn = (double)T(x).H * T(x).W;
    net->attn_flops += 4.0 * Tn * Tn * C;
    net->act_bytes += (4.0 * C * Tn) * esz;
    return add_conv(p + ".proj_out", op.dst, -1, C, C, 1, CONV_UNIT, true, 0, 0, -1, x, RES_SAME, OUT_NHWC);
  }

  int resample(int x, int mode) {
    PlanOp op; op.kind = OP_RESAMPLE; op.src0 = x; op.mode = mode;
    const int Ho = mode == CONV_UP2 ? T(x).H * 2 : T(x).H / 2, Wo = mode == CONV_UP2 ? T(x).W * 2 : T(x).W / 2;
    op.dst = tensor(T(x).C, Ho, Wo);
    net->ops.push_back(op);
    return op.dst;
  }

  int walk() {
    const int mc = cfg.model_channels, S = cfg.image_size;
    net->in_pad = (int)align_up(cfg.in_channels, CH);
    net->te_w0 = put_linear_t("time_embed.0.weight", 4 * mc, mc);
    net->te_b0 = put_f32("time_embed.0.bias", {4 * mc});
    net->te_w2 = put_linear_t("time_embed.2.weight", 4 * mc, 4 * mc);
    net->te_b2 = put_f32("time_embed.2.bias", {4 * mc});
    if (cfg.num_classes > 0) {   // UNetModel.label_emb (unet.py:571-572): nn.Embedding(num_classes, 4 mc), rows as they are
      net->num_classes = cfg.num_classes;
      net->label_w = put_f32("label_emb.weight", {cfg.num_classes, 4 * mc});
    }
    net->in_tensor = tensor(net->in_pad, S, S);
    int h = net->in_tensor;
    std::vector<int> hs;
    bool in_open = true;   // the next block of the list opens an input_blocks[i] (each ends with its push)
    for (const Block& b : unet_blocks(cfg)) {
      int skip = -1;
      if (b.pop) { skip = hs.back(); hs.pop_back(); }
      // the model's block boundaries (feature reuse, unet_cache_range): input_blocks[i] runs from here to its push, output_blocks[i] opens with its pop
      const bool opens_in = in_open && b.prefix.rfind("input_blocks.", 0) == 0;
      if (opens_in || b.pop) {
        (b.pop ? net->out_block_op : net->in_block_op).push_back((int)net->ops.size());
        (b.pop ? net->out_block_flops : net->in_block_flops).push_back(net->conv_flops + net->attn_flops);
        if (b.pop) net->out_block_h.push_back(h);
        in_open = false;
      }
      switch (b.kind) {
        case BLK_CONV_IN: h = add_conv(b.prefix, h, -1, b.cin, b.cout, 3, CONV_UNIT, false, 0, 0, -1, -1, RES_NONE, OUT_NHWC); break;
        case BLK_RES: h = res_block(b.prefix, h, skip, b.cin, b.cout, b.dir > 0, b.dir < 0); break;
        case BLK_ATTN: h = attn_block(b.prefix, h, b.cout, heads_for(b.cout, b.upsample)); break;
        case BLK_RESAMPLE_CONV:
          h = add_conv(b.prefix, h, -1, b.cin, b.cout, 3, b.dir > 0 ? CONV_UP2 : CONV_STRIDE2, false, 0, 0, -1, -1, RES_NONE, OUT_NHWC);
          break;
        case BLK_RESAMPLE: h = resample(h, b.dir > 0 ? CONV_UP2 : CONV_POOL2); break;
        case BLK_OUT:
          add_gn(h, -1, b.prefix + ".0.weight", b.prefix + ".0.bias", -1, 1, false);
          add_conv(b.prefix + ".2", h, -1, b.cin, b.cout, 3, CONV_UNIT, false, 1, 1, -1, -1, RES_NONE, OUT_NCHW_F32);
          break;
      }
      if (!err.empty()) return -1;
      if (b.push) { hs.push_back(h); in_open = true; }
    }
    // batched emb_layers: Wt [4mc][emb_total], bias [emb_total]
    const int K = 4 * mc;
    net->emb_total = emb_total;
    net->emb_w = alloc((size_t)K * emb_total * 4);
    net->emb_b = alloc((size_t)emb_total * 4);
    if (!dry) {
      float* W = reinterpret_cast<float*>(blob.data() + net->emb_w);
      float* Bv = reinterpret_cast<float*>(blob.data() + net->emb_b);
      for (auto& e : emb_parts) {
        const float* w = host[pidx[e.name + ".weight"]];
        const float* b = host[pidx[e.name + ".bias"]];
        for (int j = 0; j < e.width; ++j) {
          Bv[e.off + j] = b[j];
          for (int k = 0; k < K; ++k) W[(size_t)k * emb_total + e.off + j] = w[(size_t)j * K + k];
        }
      }
    }
    net->conv_flops += 2.0 * (double)K * emb_total + 2.0 * (double)mc * K + 2.0 * (double)K * K;
    net->out_channels = cfg.out_channels;
    net->launches = 5 + (int64_t)net->ops.size();
    return 0;
  }
};

int check_cfg(const mi355_unet_config& c) {
  MI355_REQUIRE(c.dtype == MI355_F32 || c.dtype == MI355_BF16 || c.dtype == MI355_BF16X2 || c.dtype == MI355_F16, -1,
                "unet: dtype must be MI355_F32, MI355_BF16, MI355_BF16X2 or MI355_F16");
  MI355_REQUIRE(!((c.dtype == MI355_BF16X2 || c.dtype == MI355_F16) && c.differentiable), -4, "unet: MI355_BF16X2 / MI355_F16 plans have no backward pass");
  MI355_REQUIRE(c.n_channel_mult >= 1 && c.n_channel_mult <= 8 && c.n_attention_ds >= 0 && c.n_attention_ds <= 8, -1, "unet: bad config arrays");
  MI355_REQUIRE(c.model_channels % 32 == 0 && c.model_channels > 0, -4, "unet: model_channels must be a multiple of 32 (GroupNorm32 + 64-byte channel chunks)");
  MI355_REQUIRE(c.in_channels > 0 && c.in_channels <= 32 && c.out_channels > 0 && c.out_channels <= 32, -4, "unet: in/out channels must be in 1..32");
  MI355_REQUIRE(c.image_size > 0 && c.num_res_blocks > 0, -1, "unet: bad sizes");
  MI355_REQUIRE(c.num_classes >= 0, -1, "unet: num_classes must be >= 0 (0: no label embedding)");
  return 0;
}

}  // namespace

int unet_enumerate_params(const mi355_unet_config& cfg, std::vector<ParamInfo>& out) {
  if (int rc = check_cfg(cfg)) return rc;
  out.clear();
  const int mc = cfg.model_channels, E = 4 * mc;
  auto add = [&](const std::string& n, std::vector<int64_t> s) { out.push_back({n, s}); };
  auto conv = [&](const std::string& p, int co, int ci, int k) { add(p + ".weight", {co, ci, k, k}); add(p + ".bias", {co}); };
  auto res = [&](const std::string& p, int cin, int cout) {
    add(p + ".in_layers.0.weight", {cin}); add(p + ".in_layers.0.bias", {cin});
    conv(p + ".in_layers.2", cout, cin, 3);
    const int ew = cfg.use_scale_shift_norm ? 2 * cout : cout;
    add(p + ".emb_layers.1.weight", {ew, E}); add(p + ".emb_layers.1.bias", {ew});
    add(p + ".out_layers.0.weight", {cout}); add(p + ".out_layers.0.bias", {cout});
    conv(p + ".out_layers.3", cout, cout, 3);
    if (cin != cout) conv(p + ".skip_connection", cout, cin, 1);
  };
  auto attn = [&](const std::string& p, int C) {
    add(p + ".norm.weight", {C}); add(p + ".norm.bias", {C});
    add(p + ".qkv.weight", {3 * C, C, 1}); add(p + ".qkv.bias", {3 * C});
    add(p + ".proj_out.weight", {C, C, 1}); add(p + ".proj_out.bias", {C});
  };
  add("time_embed.0.weight", {E, mc}); add("time_embed.0.bias", {E});
  add("time_embed.2.weight", {E, E}); add("time_embed.2.bias", {E});
  if (cfg.num_classes > 0) add("label_emb.weight", {cfg.num_classes, E});
  for (const Block& b : unet_blocks(cfg)) {
    switch (b.kind) {
      case BLK_CONV_IN: case BLK_RESAMPLE_CONV: conv(b.prefix, b.cout, b.cin, 3); break;
      case BLK_RES: res(b.prefix, b.cin, b.cout); break;
      case BLK_ATTN: attn(b.prefix, b.cout); break;
      case BLK_RESAMPLE: break;
      case BLK_OUT: add(b.prefix + ".0.weight", {b.cin}); add(b.prefix + ".0.bias", {b.cin}); conv(b.prefix + ".2", b.cout, b.cin, 3); break;
    }
  }
  return 0;
}

// apply-type GroupNorm site (small images): writes silu?(GN(x)) for a prologue-free consumer, and may be applied by its producers' epilogues
static bool apply_site(const PlanOp& o) { return o.kind == OP_GN && o.dst >= 0 && o.gn_site < 0; }

// What the forward resolver takes for granted about a plan, checked once where the plan is made: a tensor is read by at most two apply-type
// sites (the next block's norm and, for a skip, the up path's concat norm), and the conv that can carry a 1x1 skip conv is the next op.
static int check_plan(const mi355_unet* net) {
  std::vector<char> n_sites(net->tensors.size(), 0);
  for (size_t j = 0; j < net->ops.size(); ++j) {
    const PlanOp& o = net->ops[j];
    if (apply_site(o))
      for (int s : {o.src0, o.src1}) MI355_REQUIRE(s < 0 || ++n_sites[s] <= 2, -4, "unet plan: a tensor is read by more than two apply-type GroupNorm sites");
    MI355_REQUIRE(o.carrier < 0 || ((size_t)o.carrier == j + 1 && net->ops[j + 1].kind == OP_CONV && net->ops[j + 1].skip_op == (int)j), -4,
                  "unet plan: a skip conv's carrier is not the next op");
  }
  return 0;
}

int unet_cache_branches(const mi355_unet* net) { return (int)net->in_block_op.size() - 1; }
int unet_cache_range(const mi355_unet* net, int k, int* lo, int* hi, int* tensor) {
  const int n = (int)net->in_block_op.size();
  MI355_REQUIRE(k >= 1 && k <= n - 1, -1, "feature cache: branch must be in 1.." + std::to_string(n - 1) + " for this net (got " + std::to_string(k) + ")");
  if (lo) *lo = net->in_block_op[k];
  if (hi) *hi = net->out_block_op[n - k];
  if (tensor) *tensor = net->out_block_h[n - k];
  return 0;
}
double unet_cache_retained_share(const mi355_unet* net, int k) {
  const int n = (int)net->in_block_op.size();
  const double total = net->conv_flops + net->attn_flops;
  return total > 0 ? 1.0 - (net->out_block_flops[n - k] - net->in_block_flops[k]) / total : 1.0;
}
// What unet_cache_range takes for granted: as many input as output blocks, and the op in front of each output block produces the h entering it.
static int check_cache_blocks(const mi355_unet* net) {
  const size_t n = net->in_block_op.size();
  MI355_REQUIRE(n >= 1 && net->out_block_op.size() == n && net->out_block_h.size() == n, -4, "unet plan: input and output blocks do not pair up");
  for (size_t i = 0; i < n; ++i) {
    const int o = net->out_block_op[i];
    MI355_REQUIRE(o >= 1 && net->ops[o - 1].dst == net->out_block_h[i] && (i == 0 || net->in_block_op[i] > net->in_block_op[i - 1]), -4,
                  "unet plan: the op in front of an output block does not produce its input");
  }
  return 0;
}

static int run_walker(const mi355_unet_config& cfg, const float* const* host, mi355_unet* net, Walker& w) {
  // MI355_BF16X2 = bf16 storage and MFMAs with every conv / qkv weight held as hi + lo bf16 halves: from here on the plan is a bf16 plan with wsplit set
  // and MI355_F16 -> DT_F16: net->cfg.dtype holds the INTERNAL element-type code (ops.h) from here on
  net->wsplit = cfg.dtype == MI355_BF16X2 ? 1 : 0;
  w.cfg = cfg; w.cfg.dtype = cfg.dtype == MI355_F16 ? DT_F16 : (net->wsplit ? DT_BF16 : cfg.dtype);
  w.dtype = w.cfg.dtype; w.esz = w.dtype == 0 ? 4 : 2; w.CH = w.dtype == 0 ? 16 : 32;
  w.dry = host == nullptr; w.host = host; w.net = net;
  if (int rc = unet_enumerate_params(cfg, w.params)) return rc;
  for (size_t i = 0; i < w.params.size(); ++i) w.pidx[w.params[i].name] = (int)i;
  net->cfg = w.cfg;
  net->knobs = cfg.debug ? *cfg.debug : mi355_default_debug();
  net->cfg.debug = nullptr;
  if (w.walk() != 0 || !w.err.empty()) { mi355_set_error("unet plan: " + w.err); return -4; }
  if (int rc = check_plan(net)) return rc;
  return check_cache_blocks(net);
}

int64_t unet_plan_dry(const mi355_unet_config& cfg, mi355_unet* net) {
  Walker w;
  if (int rc = run_walker(cfg, nullptr, net, w)) return rc;
  return (int64_t)w.cursor;
}
int64_t unet_weight_bytes(const mi355_unet_config& cfg) {
  mi355_unet tmp;
  return unet_plan_dry(cfg, &tmp);
}

int unet_build(const mi355_unet_config& cfg, const float* const* params_host, int n_params, void* dev_weights,
               int64_t dev_weights_bytes, hipStream_t stream, mi355_unet** out) {
  MI355_REQUIRE(params_host && dev_weights && out, -1, "unet_create: null argument");
  mi355_unet* net = new mi355_unet();
  Walker w;
  int rc = run_walker(cfg, params_host, net, w);
  if (rc == 0 && n_params != (int)w.params.size()) { mi355_set_error("unet_create: parameter count mismatch"); rc = -2; }
  if (rc == 0 && (int64_t)w.cursor > dev_weights_bytes) { mi355_set_error("unet_create: device weight buffer too small"); rc = -2; }
  if (rc == 0) {
    hipError_t e = hipMemcpyAsync(dev_weights, w.blob.data(), w.cursor, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);  // blob is a temporary: creation is a one-off, not a hot path
    if (e != hipSuccess) { mi355_set_error(std::string("unet_create: weight upload: ") + hipGetErrorString(e)); rc = -3; }
  }
  if (rc == 0) {
    hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&net->err_host), 64, hipHostMallocMapped);
    if (e == hipSuccess) { *net->err_host = 0u; e = hipHostGetDevicePointer(reinterpret_cast<void**>(&net->err_dev), net->err_host, 0); }
    if (e != hipSuccess) { (void)hipGetLastError(); mi355_set_error(std::string("unet_create: pinned error word: ") + hipGetErrorString(e)); rc = -3; }
  }
  if (rc) { delete net; return rc; }
  net->params = w.params;
  net->tensor_state_n = net->tensors.size();
  net->tensor_state.reset(new std::atomic<char>[net->tensor_state_n]);
  for (size_t i = 0; i < net->tensor_state_n; ++i) net->tensor_state[i].store(0, std::memory_order_relaxed);
  net->dev_weights = reinterpret_cast<char*>(dev_weights);
  net->dev_weights_bytes = (int64_t)w.cursor;
  *out = net;
  return 0;
}

mi355_unet::~mi355_unet() {
  if (err_host) (void)hipHostFree(err_host);
  for (auto& g : graphs) if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (capture_stream) (void)hipStreamDestroy(capture_stream);
}

int unet_status(const mi355_unet* net, int clear) {
  if (!net || !net->err_host) return 0;
  const uint32_t v = *reinterpret_cast<volatile uint32_t*>(net->err_host);
  if (clear) *reinterpret_cast<volatile uint32_t*>(net->err_host) = 0u;
  if (v == 0u) return 0;
  if (!(v & 1u)) {   // bit 1 alone: a label kernel met a class label outside [0, num_classes)
    mi355_set_error("a launch of this handle was given a class label outside [0, num_classes) (labels of mi355_unet_forward_labels / "
                    "mi355_cfm_euler_sample_labels / mi355_sf2m_euler_sample): that image's label term was taken as zero, its output is invalid [error word " + std::to_string(v) + "]");
    return MI355_ERR_ARG;
  }
  mi355_set_error("a launch of this handle gave up a bounded counter wait of the persistent conv (hand-over stalled): its output is invalid"
                  " [error word " + std::to_string(v) + "]");
  return MI355_ERR_TIMEOUT;
}

WsLayout unet_ws_layout(const mi355_unet* net, int B) {
  const int mc = net->cfg.model_channels, esz = net->cfg.dtype == 0 ? 4 : 2, CH = net->cfg.dtype == 0 ? 16 : 32;
  WsLayout l{}; size_t c = 0;
  auto take = [&](size_t bytes) { size_t o = c; c = align_up(c + bytes, 256); return o; };
  l.temb = take((size_t)B * mc * 4);
  l.emb1 = take((size_t)B * 4 * mc * 4);
  l.emb2 = take((size_t)B * 4 * mc * 4);
  l.embp = take((size_t)B * net->emb_total * 4);
  l.gna = take((size_t)B * net->max_gn_c * 4);
  l.gnb = take((size_t)B * net->max_gn_c * 4);
  l.stats = take((size_t)B * net->stats_floats_per_image * 4);
  l.sites = take((size_t)B * net->site_floats_per_image * 4);
  l.arena = take(net->act_elems_per_image * (size_t)B * esz);
  if (net->cfg.differentiable) {   // backward scratch: one gradient per activation tensor + the temporaries sized by the plan
    const size_t S = (size_t)net->cfg.image_size * net->cfg.image_size;
    l.grads = take(net->act_elems_per_image * (size_t)B * esz);
    l.du = take(net->bwd_du_elems * (size_t)B * esz);
    l.tmp = take(net->bwd_tmp_elems * (size_t)B * esz);
    l.z = take(net->bwd_z_elems * (size_t)B * esz);
    l.dy = take(S * CH * (size_t)B * esz);
    l.ld = take(net->bwd_ld_floats * (size_t)B * 4);
  }
  l.total = c;
  return l;
}

int unet_embedding_table(const mi355_unet* net, const float* t_dev, int n, float* table, float* scratch, hipStream_t stream) {
  const int mc = net->cfg.model_channels;
  const char* W = net->dev_weights;
  auto WF = [&](size_t off) { return reinterpret_cast<const float*>(W + off); };
  float* temb = scratch; float* e1 = scratch + (size_t)n * mc; float* e2 = e1 + (size_t)n * 4 * mc;
  int rc;
  // emb2 = silu(time_embed(timestep_embedding(t))): the SiLU that opens every emb_layers is applied once here
  if ((rc = timestep_embedding_launch(t_dev, n, mc, 10000.f, temb, stream))) return rc;
  if ((rc = linear_launch(temb, WF(net->te_w0), WF(net->te_b0), e1, n, mc, 4 * mc, 0, 1, stream))) return rc;
  if ((rc = linear_launch(e1, WF(net->te_w2), WF(net->te_b2), e2, n, 4 * mc, 4 * mc, 0, 1, stream))) return rc;
  return linear_launch(e2, WF(net->emb_w), WF(net->emb_b), table, n, 4 * mc, net->emb_total, 0, 0, stream);
}

int unet_embedding_rows_labels(const mi355_unet* net, const float* t_dev, int n_t, const int32_t* labels, int R, int h_div, float* table,
                               float* scratch, hipStream_t stream) {
  MI355_REQUIRE(net->num_classes > 0 && net->label_w, -1, "class labels given to a net built without num_classes");
  const int mc = net->cfg.model_channels;
  const char* W = net->dev_weights;
  auto WF = [&](size_t off) { return reinterpret_cast<const float*>(W + off); };
  float* temb = scratch; float* e1 = scratch + (size_t)n_t * mc; float* e2 = e1 + (size_t)n_t * 4 * mc;
  int rc;
  // e2 = time_embed(timestep_embedding(t)) WITHOUT the SiLU: with labels it follows the add (label_emb_linear's prologue)
  if ((rc = timestep_embedding_launch(t_dev, n_t, mc, 10000.f, temb, stream))) return rc;
  if ((rc = linear_launch(temb, WF(net->te_w0), WF(net->te_b0), e1, n_t, mc, 4 * mc, 0, 1, stream))) return rc;
  if ((rc = linear_launch(e1, WF(net->te_w2), WF(net->te_b2), e2, n_t, 4 * mc, 4 * mc, 0, 0, stream))) return rc;
  return label_emb_linear_launch(e2, h_div, WF(net->label_w), labels, net->num_classes, WF(net->emb_w), WF(net->emb_b), table, R, 4 * mc,
                                 net->emb_total, net->err_dev, stream);
}

int64_t unet_workspace_bytes(const mi355_unet* net, int batch) { return (int64_t)unet_ws_layout(net, batch).total; }

// ---- resolve ---------------------------------------------------------------------------------------------------------------------------
namespace {

// Walks the plan once, in order, deciding what each op becomes in this forward.  All of a forward's bookkeeping lives here.
struct Resolver {
  const mi355_unet* net; const WsView& v; const UnetRun& run; const int B;
  const float* x; int Cx; const float* cond; int Cc; float* out;
  const float* embp; int estride;
  struct OpState {
    char gn_done = 0;      // GroupNorm site its producers' epilogues applied (small levels: ConvDesc::act_out; 16x16: in place)
    char pro_off = 0;      // conv whose input arrives already normalised (16x16 level: applied IN PLACE by the producer)
    char site_parts = 0;   // how many of an apply-type site's sources their producers have applied so far
  };
  struct TensorState {
    int readers = 0;
    int gn_slots = 0;      // partial-statistics slots the tensor's producer filled in THIS forward
    int n_sites = 0, sites[2] = {-1, -1};   // apply-type GroupNorm sites (small images) that read it: the next block's norm and, for a skip, the concat's
  };
  std::vector<OpState> ops;
  std::vector<TensorState> tens;

  const float* WF(size_t off) const { return reinterpret_cast<const float*>(net->dev_weights + off); }
  int cin(const PlanOp& op) const { return net->tensors[op.src0].C + (op.src1 >= 0 ? net->tensors[op.src1].C : 0); }

  void count_readers() {   // (at most two sites per tensor, a skip conv's carrier the next op: check_plan, at build)
    ops.assign(net->ops.size(), OpState());
    tens.assign(net->tensors.size(), TensorState());
    for (size_t j = 0; j < net->ops.size(); ++j) {
      const PlanOp& o = net->ops[j];
      if (o.src0 >= 0) ++tens[o.src0].readers;
      if (o.src1 >= 0) ++tens[o.src1].readers;
      if (o.kind == OP_CONV && o.res >= 0) ++tens[o.res].readers;
      if (apply_site(o)) {
        for (int s : {o.src0, o.src1}) if (s >= 0) tens[s].sites[tens[s].n_sites++] = (int)j;
      }
    }
  }

  // the conv a GroupNorm pass feeds is the next op of the plan: the pass warms the L2s with its weights (common.h l2_warm_wave)
  // knobs.l2_warm: 1 = statistics / apply passes, 2 = finalize passes (measured: no gain, off)
  void warm_next(size_t oi, const void*& wp, uint32_t& wb, int bit) const {
    if (!(net->knobs.l2_warm & bit) || oi + 1 >= net->ops.size() || net->ops[oi + 1].kind != OP_CONV) return;
    const PlanOp& nx = net->ops[oi + 1];
    wp = net->dev_weights + nx.w_off; wb = (uint32_t)conv_packed_weight_bytes(net->cfg.dtype, nx.Cout, cin(nx), nx.ks, net->wsplit);
  }

  // The whole description of plan conv oi, everything it may do included; conv_route says which of it the launch does.  skip: with its
  // ResBlock's 1x1 skip conv (op.skip_op) riding along.  ConvSites: the GroupNorm sites act_out / act2_out stand for.
  struct ConvSites { size_t act_consumer = 0; int fused[2] = {-1, -1}; };
  void describe_conv(size_t oi, bool skip, ConvDesc& c, ConvSites& r) const {
    const PlanOp& op = net->ops[oi];
    const PlanTensor& s0 = net->tensors[op.src0];
    c.dtype = net->cfg.dtype; c.src0 = v.tensor(op.src0); c.C0 = s0.C; c.src1 = v.tensor(op.src1); c.C1 = op.src1 >= 0 ? net->tensors[op.src1].C : 0;
    c.N = B; c.Hs = s0.H; c.Ws = s0.W; c.mode = op.mode; c.ks = op.ks; c.wsplit = net->wsplit;
    if (op.use_pro && !ops[oi].pro_off) {
      c.pro_a = v.f32(v.l.gna); c.pro_b = v.f32(v.l.gnb); c.pro_silu = op.pro_silu;
      if (op.gn_site >= 0) { const WsView::Site s = v.site(op.gn_site); c.pro_a = s.a; c.pro_b = s.b; }
    }
    c.w = net->dev_weights + op.w_off; c.bias = WF(op.bias_off); c.Cout = op.Cout;
    if (op.has_wu) c.w_up2 = net->dev_weights + op.wu_off;
    if (op.src0 == net->in_tensor) {
      c.cin_real = net->cfg.in_channels;
      // the first conv may read the caller's fp32 NCHW tensors itself (conv_edge bit 2): no packed copy, no pack launch
      if (!net->cfg.differentiable && tens[net->in_tensor].readers == 1) { c.nchw0 = x; c.nchw_c0 = Cx; c.nchw1 = cond; c.nchw_c1 = cond ? Cc : 0; }
    }
    if (op.out_mode == OUT_NCHW_F32 && run.euler_x) { c.axpy_x = run.euler_x; c.axpy_scale = run.euler_dt; }
    if (op.emb_off >= 0) { c.emb = embp + op.emb_off; c.emb_stride = estride; }
    if (op.res >= 0) { c.res = v.tensor(op.res); c.res_mode = op.res_mode; }
    c.out_mode = op.out_mode;
    c.knobs = &net->knobs; c.err = net->err_dev;
    c.out = op.out_mode == OUT_NHWC ? v.tensor(op.dst) : (void*)out;
    if (skip) {
      const PlanOp& sk = net->ops[op.skip_op];
      c.skip_src0 = v.tensor(sk.src0); c.skip_C0 = net->tensors[sk.src0].C;
      c.skip_src1 = v.tensor(sk.src1); c.skip_C1 = sk.src1 >= 0 ? net->tensors[sk.src1].C : 0;
      c.w = net->dev_weights + op.wf_off; c.bias = WF(op.bf_off); c.res = nullptr; c.res_mode = RES_NONE;
    }
    if (op.dst >= 0 && net->tensors[op.dst].stats_cap) { c.gn_stats = v.stats(op.dst); c.gn_slots_cap = net->tensors[op.dst].stats_cap; }
    if (op.dst >= 0 && op.out_mode == OUT_NHWC && op.res < 0 && oi + 2 < net->ops.size() && tens[op.dst].readers == 2) {
      // statistics-type site (larger images) read by exactly one prologue conv: where the persistent kernel's tile is the whole
      // image (16x16) it normalises its own output in place, the site's launch disappears and the consumer runs prologue-free
      const PlanOp& g = net->ops[oi + 1];
      if (g.kind == OP_GN && g.fin_ok && g.dst < 0 && g.src0 == op.dst && g.src1 < 0 && g.gn_site < 0) {
        for (size_t j = oi + 2; j < net->ops.size() && j <= oi + 3; ++j) {
          const PlanOp& cn = net->ops[j];
          if (cn.kind == OP_CONV && cn.use_pro && cn.src0 == op.dst && cn.src1 < 0 && cn.gn_site < 0) { r.act_consumer = j; break; }
        }
        if (r.act_consumer) {
          c.act_out = c.out; c.act_raw = 0; c.act_gamma = WF(g.gamma_off); c.act_beta = WF(g.beta_off);
          if (g.film_emb_off >= 0) { c.act_film = embp + g.film_emb_off; c.act_film_stride = estride; }
          c.act_silu = net->ops[r.act_consumer].pro_silu;
        }
      }
    }
    if (!c.act_out && op.dst >= 0 && op.out_mode == OUT_NHWC) {
      // The apply-type GroupNorm sites (small images) that read this conv's output: the one that follows it (in_layers / out_layers norm of
      // the next conv, unet.py:196-212) and, for a skip connection, the norm of the up path's concat (unet.py:650), whose groups are whole
      // inside each source when both channel counts are multiples of the group width: each producer then applies its own channels.
      for (int k = 0; k < tens[op.dst].n_sites; ++k) {
        const int gi = tens[op.dst].sites[k];
        const PlanOp& g = net->ops[gi];
        const bool cat = g.src1 >= 0;
        const int Cg = cin(g);
        const int coff = g.src0 == op.dst ? 0 : net->tensors[g.src0].C;
        if (cat) {
          const int cpg = Cg / 32;
          if (!(net->knobs.gn_epilogue & 4) || g.film_emb_off >= 0 || g.src0 == g.src1 || Cg % 32 || net->tensors[g.src0].C % cpg || net->tensors[g.src1].C % cpg) continue;
        }
        if (!c.act_out) {
          c.act_out = v.tensor(g.dst); c.act_gamma = WF(g.gamma_off) + coff; c.act_beta = WF(g.beta_off) + coff;
          if (g.film_emb_off >= 0) { c.act_film = embp + g.film_emb_off; c.act_film_stride = estride; }
          c.act_silu = g.pro_silu; c.act_stride = Cg; c.act_coff = coff; c.act_cpg = Cg / 32;
          if (!cat || coff == 0) warm_next((size_t)gi, c.warm, c.warm_bytes, 1);
          r.fused[0] = gi;
        } else if (!c.act2_out && g.film_emb_off < 0) {
          c.act2_out = v.tensor(g.dst); c.act2_gamma = WF(g.gamma_off) + coff; c.act2_beta = WF(g.beta_off) + coff;
          c.act2_silu = g.pro_silu; c.act2_stride = Cg; c.act2_coff = coff; c.act2_cpg = Cg / 32;
          r.fused[1] = gi;
        }
      }
      // the raw tensor is written unless the one site asked for is its only reader (with two sites asked for the launch may still take one)
      if (c.act_out) c.act_raw = c.act2_out ? 1 : tens[op.dst].readers > 1;
    }
  }
  // what the routed launch of conv oi settles for the ops behind it
  void settle_conv(size_t oi, const ConvRoute& rt, const ConvSites& r) {
    if (rt.act_done && r.act_consumer) { ops[oi + 1].gn_done = 1; ops[r.act_consumer].pro_off = 1; }
    else if (rt.act_done) {
      for (int k = 0; k < 2; ++k) {
        if (!(rt.act_done & (1 << k)) || r.fused[k] < 0) continue;
        if (++ops[r.fused[k]].site_parts == (net->ops[r.fused[k]].src1 >= 0 ? 2 : 1)) ops[r.fused[k]].gn_done = 1;
      }
    }
    if (net->ops[oi].dst >= 0) tens[net->ops[oi].dst].gn_slots = rt.gn_slots;
  }

  // a GroupNorm op's affine parameters and, under use_scale_shift_norm, its FiLM rows
  void gn_common(const PlanOp& op, const float*& gamma, const float*& beta, const float*& film, int& film_stride) const {
    gamma = WF(op.gamma_off); beta = WF(op.beta_off);
    if (op.film_emb_off >= 0) { film = embp + op.film_emb_off; film_stride = estride; }
  }
  GnFinDesc describe_gn_finalize(size_t oi) const {
    const PlanOp& op = net->ops[oi];
    const PlanTensor& s0 = net->tensors[op.src0];
    GnFinDesc g; g.stats0 = v.stats(op.src0); g.slots0 = tens[op.src0].gn_slots; g.C0 = s0.C;
    if (op.src1 >= 0) { g.stats1 = v.stats(op.src1); g.slots1 = tens[op.src1].gn_slots; g.C1 = net->tensors[op.src1].C; }
    g.N = B; g.HW = s0.H * s0.W;
    gn_common(op, g.gamma, g.beta, g.film, g.film_stride);
    g.a = v.f32(v.l.gna); g.b = v.f32(v.l.gnb);
    g.dtype = net->cfg.dtype; g.src0 = v.tensor(op.src0); g.src1 = v.tensor(op.src1);
    warm_next(oi, g.warm, g.warm_bytes, 2);
    return g;
  }
  GnDesc describe_gn(size_t oi) const {
    const PlanOp& op = net->ops[oi];
    const PlanTensor& s0 = net->tensors[op.src0];
    GnDesc g; g.dtype = net->cfg.dtype; g.src0 = v.tensor(op.src0); g.C0 = s0.C; g.src1 = v.tensor(op.src1); g.C1 = op.src1 >= 0 ? net->tensors[op.src1].C : 0;
    g.N = B; g.HW = s0.H * s0.W;
    gn_common(op, g.gamma, g.beta, g.film, g.film_stride);
    g.a = v.f32(v.l.gna); g.b = v.f32(v.l.gnb);
    if (op.gn_site >= 0) { const WsView::Site s = v.site(op.gn_site); g.a = s.a; g.b = s.b; g.mean = s.mean; g.rstd = s.rstd; }   // differentiable plan: this site's own
    if (op.dst >= 0) { g.y = v.tensor(op.dst); g.y_silu = op.pro_silu; }
    warm_next(oi, g.warm, g.warm_bytes, 1);
    return g;
  }
  AttnDesc describe_attn(const PlanOp& op) const {
    const PlanTensor& s0 = net->tensors[op.src0];
    AttnDesc a; a.dtype = net->cfg.dtype; a.qkv = v.tensor(op.src0); a.out = v.tensor(op.dst); a.N = B; a.T = s0.H * s0.W;
    a.heads = op.heads; a.ch = op.ch; a.new_order = net->cfg.use_new_attention_order;
    return a;
  }
  AttnFusedDesc describe_attn_fused(const PlanOp& op) const {
    const PlanTensor& s0 = net->tensors[op.src0];
    AttnFusedDesc a; a.dtype = net->cfg.dtype; a.x = v.tensor(op.src0); a.ga = v.f32(v.l.gna); a.gb = v.f32(v.l.gnb);
    a.w = net->dev_weights + op.w_off; a.bias = WF(op.bias_off);
    a.out = v.tensor(op.dst); a.N = B; a.T = s0.H * s0.W; a.C = s0.C; a.heads = op.heads; a.ch = op.ch;
    a.new_order = net->cfg.use_new_attention_order; a.knobs = &net->knobs;
    return a;
  }
  PoolAffStep describe_pool(const PlanOp& op) const {
    const PlanTensor& s0 = net->tensors[op.src0];
    PoolAffStep p{net->cfg.dtype, v.tensor(op.src0), v.f32(v.l.gna), v.f32(v.l.gnb), op.pro_silu, v.tensor(op.dst), B, s0.H, s0.W, s0.C};
    if (op.gn_site >= 0) { const WsView::Site s = v.site(op.gn_site); p.a = s.a; p.b = s.b; }
    return p;
  }

  static ConvStep& push_conv(ResolvedForward* f) { return std::get<ConvStep>(f->steps.emplace_back(std::in_place_type<ConvStep>)); }

  int resolve(ResolvedForward* f) {
    count_readers();
    const size_t n = net->ops.size();
    f->steps.clear();
    f->steps.reserve(n);
    // steps are described and routed in place.  carried: the previous op was a 1x1 skip conv whose probe the route took, so this op's step
    // (its ResBlock's second conv) is already there; `sites` are that description's.
    bool carried = false;
    ConvSites sites;
    for (size_t oi = 0; oi < n; ++oi) {
      const PlanOp& op = net->ops[oi];
      const PlanTensor& s0 = net->tensors[op.src0];
      switch (op.kind) {
        case OP_GN:
          if (ops[oi].gn_done) f->steps.emplace_back(GnAbsorbed{});
          else if (op.fin_ok && op.dst < 0 && tens[op.src0].gn_slots > 0 && (op.src1 < 0 || tens[op.src1].gn_slots > 0)) f->steps.emplace_back(describe_gn_finalize(oi));
          else f->steps.emplace_back(describe_gn(oi));
          break;
        case OP_CONV: {
          if (!carried && op.carrier >= 0) {
            // 1x1 skip_connection of a ResBlock whose plan names a carrier (small levels, 128-channel large levels): does the second conv's launch take it along?  The carrier is the next op and
            // nothing it is described from changes in between, so the probe's description and route are that step's.
            f->steps.emplace_back(ConvCarried{});
            ConvStep& c2 = push_conv(f);
            sites = ConvSites();
            describe_conv(oi + 1, true, c2.c, sites);
            if (conv_route(c2.c, &c2.rt) == 0) { carried = true; break; }
            f->steps.pop_back(); f->steps.pop_back();   // declined: both convs are launched on their own
          }
          if (!carried) {
            ConvStep& st = push_conv(f);
            sites = ConvSites();
            describe_conv(oi, false, st.c, sites);
            if (int rc = conv_route(st.c, &st.rt)) return rc;
          }
          carried = false;
          const ConvRoute& rt = std::get<ConvStep>(f->steps[oi]).rt;
          settle_conv(oi, rt, sites);
          if (rt.axpy) f->euler_in_conv = true;
          if (op.src0 == net->in_tensor && rt.reads_nchw) f->pack = false;
          break;
        }
        case OP_ATTN: f->steps.emplace_back(describe_attn(op)); break;
        case OP_ATTN_FUSED: f->steps.emplace_back(describe_attn_fused(op)); break;
        case OP_POOLAFF: f->steps.emplace_back(describe_pool(op)); break;
        default: f->steps.emplace_back(ResampleStep{net->cfg.dtype, v.tensor(op.src0), v.tensor(op.dst), B, s0.H, s0.W, s0.C, op.mode}); break;
      }
    }
    return 0;
  }
};

template <typename T> bool is(const ForwardStep& s) { return std::holds_alternative<T>(s); }

// ---- issue: one launch per descriptor type ---------------------------------------------------------------------------------------------
int issue(const GnAbsorbed&, hipStream_t) { return 0; }
int issue(const ConvCarried&, hipStream_t) { return 0; }
int issue(const GnFinDesc& g, hipStream_t s) { return gn_finalize_launch(g, s); }
int issue(const GnDesc& g, hipStream_t s) { return gn_affine_launch(g, s); }
int issue(const ConvStep& c, hipStream_t s) { return conv_launch(c.c, c.rt, s); }
int issue(const AttnDesc& a, hipStream_t s) { return attention_launch(a, s); }
int issue(const AttnFusedDesc& a, hipStream_t s) { return attn_fused_launch(a, s); }
int issue(const PoolAffStep& p, hipStream_t s) { return affine_pool_launch(p.dtype, p.in, p.a, p.b, p.silu, p.out, p.N, p.H, p.W, p.C, s); }
int issue(const ResampleStep& r, hipStream_t s) { return resample_launch(r.dtype, r.in, r.out, r.N, r.H, r.W, r.C, r.mode, s); }

// The mi355_op_profile record (all but ms) of plan op `op` as step `st` ran it at batch B.  tile -1, -1: nothing was launched for this op.
mi355_op_profile profile_record(const mi355_unet* net, const PlanOp& op, const ForwardStep& st, int B) {
  mi355_op_profile r{};
  const PlanTensor& s0 = net->tensors[op.src0];
  const int cin = s0.C + (op.src1 >= 0 ? net->tensors[op.src1].C : 0), esz = net->cfg.dtype == 0 ? 4 : 2;
  r.h = s0.H; r.w = s0.W;
  if (!unet_step_launches(st)) r.tile_m = r.tile_n = -1;
  switch (op.kind) {
    case OP_GN:
      r.kind = MI355_OP_GN; r.cin = cin;
      // absorbed / finalized: no activation traffic (the statistics came with the producers' epilogues)
      if (is<GnDesc>(st)) r.bytes = (double)B * s0.H * s0.W * cin * esz * (op.dst >= 0 ? 2 : 1);
      break;
    case OP_CONV: {
      r.kind = MI355_OP_CONV; r.ks = op.ks; r.cin = cin; r.cout = op.Cout;
      if (!is<ConvStep>(st)) break;
      const ConvStep& c = std::get<ConvStep>(st);
      const ConvGeom& cg = c.rt.geom;
      r.h = cg.Ho; r.w = cg.Wo; r.tile_m = cg.BM; r.tile_n = cg.BN;
      r.flops = 2.0 * B * cg.Ho * cg.Wo * (double)op.Cout * cin * op.ks * op.ks;
      r.bytes = ((double)B * s0.H * s0.W * cin + (double)B * cg.Ho * cg.Wo * op.Cout) * esz + (double)op.Cout * cin * op.ks * op.ks * esz;
      if (c.c.skip_src0) {   // the ResBlock's 1x1 skip conv this launch carried
        r.flops += 2.0 * B * cg.Ho * cg.Wo * (double)op.Cout * (c.c.skip_C0 + c.c.skip_C1);
        r.bytes += ((double)B * cg.Ho * cg.Wo + (double)op.Cout) * (c.c.skip_C0 + c.c.skip_C1) * esz;
      }
      break;
    }
    case OP_ATTN: {
      const int T = s0.H * s0.W;
      r.kind = MI355_OP_ATTN; r.cin = 3 * op.heads * op.ch; r.cout = op.heads * op.ch;
      r.flops = 4.0 * B * (double)T * T * op.heads * op.ch;
      r.bytes = 4.0 * B * T * op.heads * op.ch * esz;
      break;
    }
    case OP_ATTN_FUSED: {
      const int T = s0.H * s0.W;
      r.kind = MI355_OP_ATTN; r.cin = s0.C; r.cout = s0.C; r.ks = 1;   // ks = 1 marks the fused form
      r.flops = 2.0 * B * (double)T * 3.0 * s0.C * s0.C + 4.0 * B * (double)T * T * s0.C;
      r.bytes = 2.0 * B * T * (double)s0.C * esz + 3.0 * s0.C * s0.C * esz;
      break;
    }
    case OP_POOLAFF:
      r.kind = MI355_OP_RESAMPLE; r.cin = s0.C;
      r.bytes = 1.25 * B * s0.H * s0.W * (double)s0.C * esz;
      break;
    default: r.kind = MI355_OP_RESAMPLE; r.cin = s0.C; break;
  }
  return r;
}

// What the forward leaves in a step's output tensor (mi355_unet::tensor_state): 0 as the reference defines it, 1 never written, 2 normalised in place
char tensor_state_of(const ForwardStep& st) {
  if (is<ConvCarried>(st)) return 1;
  const ConvStep& c = std::get<ConvStep>(st);
  if (!c.rt.act_done) return 0;
  return c.c.act_out == c.c.out ? 2 : (c.c.act_raw ? 0 : 1);
}

}  // namespace

int unet_resolve(const WsView& v, const float* x, int Cx, const float* cond, int Cc, float* out, const UnetRun& run, ResolvedForward* f) {
  // time embedding path (fp32): emb2 = silu(time_embed(timestep_embedding(t))) ; embp = all emb_layers linears
  // in the sampler loops every image shares the step time: one embedding row, broadcast with stride 0
  // class labels: every image has its own row (estride = emb_total even for a shared t), gathered from the sampler's (step, class) table or
  // computed from t and the labels
  const mi355_unet* net = v.net;
  const int B = (int)v.B;
  const bool labelled = run.labels != nullptr;
  MI355_REQUIRE(!labelled || net->num_classes > 0, -1, "unet_forward: class labels given to a net built without num_classes");
  *f = ResolvedForward();
  f->emb = labelled ? (run.emb_row ? EMB_GATHER : EMB_LABELS) : (run.emb_row ? EMB_ROW : EMB_TIME);
  f->Be = run.t_uniform ? 1 : B; f->estride = run.t_uniform && !labelled ? 0 : net->emb_total;
  f->embp = f->emb == EMB_ROW ? run.emb_row : v.f32(v.l.embp);
  int lo = 0, hi = 0;
  if (run.reuse_branch) {   // refusals first: nothing is resolved, nothing launched
    if (int rc = unet_cache_range(net, run.reuse_branch, &lo, &hi, nullptr)) return rc;
    MI355_REQUIRE(!net->cfg.differentiable, -4, "feature cache: a differentiable plan cannot run a shallow evaluation (the backward pass would see activations of two forwards)");
  }
  Resolver r{net, v, run, B, x, Cx, cond, Cc, out, f->embp, f->estride, {}, {}};
  if (int rc = r.resolve(f)) return rc;
  f->skip_lo = (size_t)lo; f->skip_hi = (size_t)hi;
  // The cached feature is read raw across the cut (the popping ResBlock's skip conv always reads it: cin != cout over a concat), so the whole
  // forward that produced it stored it as the reference defines it; a plan in which it did not cannot be cut here.
  if (hi && (is<ConvStep>(f->steps[hi - 1]) || is<ConvCarried>(f->steps[hi - 1])))
    MI355_REQUIRE(tensor_state_of(f->steps[hi - 1]) == 0, -4, "feature cache: the producer of the cached feature does not store it as the reference defines it");
  return 0;
}

int64_t unet_launch_count(const ResolvedForward& f) {
  int64_t n = (f.emb == EMB_ROW ? 0 : f.emb == EMB_GATHER ? 1 : 4) + (f.pack ? 1 : 0);
  for (size_t i = 0; i < f.steps.size(); ++i) n += f.issued(i) && unet_step_launches(f.steps[i]);
  return n;
}

int unet_forward(const mi355_unet* net, const float* x, int Cx, const float* cond, int Cc, const float* t, float* out, int B,
                 void* workspace, int64_t workspace_bytes, hipStream_t stream, const UnetRun& run) {
  MI355_REQUIRE(net && x && t && out && workspace, -1, "unet_forward: null argument");
  MI355_REQUIRE(B > 0, -1, "unet_forward: batch must be positive");
  if (int rc = unet_status(net, 0)) return rc;   // an earlier launch of this handle gave up a counter wait
  MI355_REQUIRE(Cx + (cond ? Cc : 0) == net->cfg.in_channels, -2, "unet_forward: x/cond channels do not add up to in_channels");
  const WsView v(net, workspace, B);
  MI355_REQUIRE((int64_t)v.l.total <= workspace_bytes, -2, "unet_forward: workspace too small");
  MI355_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, -1, "unet_forward: workspace must be 256-byte aligned");
  ResolvedForward f;
  int rc;
  if ((rc = unet_resolve(v, x, Cx, cond, Cc, out, run, &f))) return rc;

  // ---- the handle's diagnostics of its most recent forward: what this forward is about to leave, known before anything is launched ----
  if (!f.pack && (size_t)net->in_tensor < net->tensor_state_n) net->tensor_state[net->in_tensor].store((char)1, std::memory_order_relaxed);
  for (size_t i = 0; i < f.steps.size(); ++i) {
    const PlanOp& op = net->ops[i];
    if (!f.issued(i)) continue;   // a shallow evaluation: the tensor keeps what the whole forward left, and its record
    if (op.kind == OP_CONV && op.dst >= 0 && (size_t)op.dst < net->tensor_state_n) net->tensor_state[op.dst].store(tensor_state_of(f.steps[i]), std::memory_order_relaxed);
  }

  // ---- issue: the prelude, then one launch per step ----
  auto mark = [&](const mi355_op_profile& r) {
    hipEvent_t e; (void)hipEventCreate(&e); (void)hipEventRecord(e, stream);
    run.prof_events->push_back(e); run.prof->push_back(r);
  };
  if (run.prof) { hipEvent_t e; (void)hipEventCreate(&e); (void)hipEventRecord(e, stream); run.prof_events->push_back(e); }
  float* rows = v.f32(v.l.embp);
  switch (f.emb) {
    case EMB_GATHER: rc = emb_gather_launch(run.emb_row, run.labels, net->num_classes, rows, B, net->emb_total, net->err_dev, stream); break;
    case EMB_LABELS: rc = unet_embedding_rows_labels(net, t, f.Be, run.labels, B, run.t_uniform ? B : 1, rows, v.f32(v.l.temb), stream); break;
    case EMB_TIME: rc = unet_embedding_table(net, t, f.Be, rows, v.f32(v.l.temb), stream); break;
    default: break;
  }
  if (rc) return rc;
  const int S = net->cfg.image_size;
  if (f.pack && (rc = pack_nhwc_launch(net->cfg.dtype, x, Cx, cond, cond ? Cc : 0, B, S * S, net->in_pad, v.tensor(net->in_tensor), stream))) return rc;
  if (run.prof) { mi355_op_profile r{}; r.kind = MI355_OP_PRELUDE; mark(r); }
  for (size_t i = 0; i < f.steps.size(); ++i) {
    if (!f.issued(i)) continue;
    if ((rc = std::visit([&](const auto& d) { return issue(d, stream); }, f.steps[i]))) return rc;
    if (run.prof) mark(profile_record(net, net->ops[i], f.steps[i], B));
  }
  if (run.euler_x && !f.euler_in_conv) {
    const int64_t n_out = (int64_t)B * net->cfg.out_channels * S * S;
    if ((rc = euler_step_launch(run.euler_x, out, run.euler_dt, n_out, stream))) return rc;
  }

  net->last_launches = unet_launch_count(f);
  return 0;
}
