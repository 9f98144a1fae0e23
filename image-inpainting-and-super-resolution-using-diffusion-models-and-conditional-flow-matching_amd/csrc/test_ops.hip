// Single-op test harness of libmi355_sampler.so (see include/mi355_sampler.h): the kernels the network launches, one op per call, NCHW fp32 at
// the boundary (mi355_conv2d / mi355_conv2d_ex, the attention ops, the GroupNorm test ops, mi355_affine_pool, mi355_grad_gather, mi355_conv2d_vjp, mi355_conv2d_fwd).
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "capi_internal.h"

extern "C" {

int64_t mi355_op_workspace_bytes(int batch, int max_channels, int hw) {
  const size_t c = (size_t)max_channels + 32;
  return (int64_t)(2 * al256((size_t)batch * hw * 4 * c * 4) + al256(c * c * 9 * 4 * 2) + 4 * al256((size_t)batch * c * 4) + (1 << 20));
}

namespace {
// device scratch of mi355_conv2d_ex's extras (a test op: plain hipMalloc, freed when the call returns)
struct ExScratch {
  std::vector<void*> ptrs;
  ~ExScratch() { for (void* q : ptrs) (void)hipFree(q); }
  void* get(size_t bytes) { void* q = nullptr; if (hipMalloc(&q, bytes ? bytes : 256) != hipSuccess) return nullptr; ptrs.push_back(q); return q; }
};
}  // namespace

static int conv2d_impl(const float* x, const float* x1, int cin1, const float* w_host, const float* bias_host, float* y, int batch, int cin,
                       int h, int w, int cout, int ksize, int stride, int resample, const float* gn_gamma, const float* gn_beta, int gn_silu,
                       const float* emb, const float* res, int res_mode, int dtype, const mi355_debug_config* debug, void* workspace,
                       int64_t workspace_bytes, void* stream, mi355_conv_extras* ex);

int mi355_conv2d(const float* x, const float* x1, int cin1, const float* w_host, const float* bias_host, float* y, int batch, int cin,
                 int h, int w, int cout, int ksize, int stride, int resample, const float* gn_gamma, const float* gn_beta, int gn_silu,
                 const float* emb, const float* res, int res_mode, int dtype, const mi355_debug_config* debug, void* workspace,
                 int64_t workspace_bytes, void* stream) {
  return conv2d_impl(x, x1, cin1, w_host, bias_host, y, batch, cin, h, w, cout, ksize, stride, resample, gn_gamma, gn_beta, gn_silu, emb, res, res_mode,
                     dtype, debug, workspace, workspace_bytes, stream, nullptr);
}
int mi355_conv2d_ex(const float* x, const float* x1, int cin1, const float* w_host, const float* bias_host, float* y, int batch, int cin,
                    int h, int w, int cout, int ksize, int stride, int resample, const float* gn_gamma, const float* gn_beta, int gn_silu,
                    const float* emb, const float* res, int res_mode, int dtype, const mi355_debug_config* debug, void* workspace,
                    int64_t workspace_bytes, void* stream, mi355_conv_extras* extras) {
  MI355_REQUIRE(extras, -1, "conv2d_ex: null extras");
  return conv2d_impl(x, x1, cin1, w_host, bias_host, y, batch, cin, h, w, cout, ksize, stride, resample, gn_gamma, gn_beta, gn_silu, emb, res, res_mode,
                     dtype, debug, workspace, workspace_bytes, stream, extras);
}

static int conv2d_impl(const float* x, const float* x1, int cin1, const float* w_host, const float* bias_host, float* y, int batch, int cin,
                       int h, int w, int cout, int ksize, int stride, int resample, const float* gn_gamma, const float* gn_beta, int gn_silu,
                       const float* emb, const float* res, int res_mode, int dtype, const mi355_debug_config* debug, void* workspace,
                       int64_t workspace_bytes, void* stream, mi355_conv_extras* ex) {

  const mi355_debug_config& K = debug ? *debug : mi355_default_debug();
  MI355_REQUIRE(x && w_host && y && workspace, -1, "conv2d: null argument");
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16 || dtype == MI355_BF16X2 || dtype == MI355_F16, -1, "conv2d: bad dtype");
  const int wsplit = dtype == MI355_BF16X2 ? 1 : 0;   // bf16 storage, weights as hi | lo bf16 halves along K
  dtype = dtype == MI355_F16 ? DT_F16 : (wsplit ? DT_BF16 : dtype);   // the internal element-type code from here on (ops.h)
  MI355_REQUIRE(stride == 1 || stride == 2, -1, "conv2d: stride must be 1 or 2");
  MI355_REQUIRE(!(stride == 2 && resample), -1, "conv2d: stride 2 cannot be combined with resampling");
  MI355_REQUIRE((x1 != nullptr) == (cin1 > 0), -1, "conv2d: x1 and cin1 go together");
  MI355_REQUIRE(res == nullptr || res_mode == RES_SAME || res_mode == RES_UP2, -1, "conv2d: res_mode must be 1 (same size) or 2 (nearest x2)");
  hipStream_t s = S(stream);
  const int CH = dtype == 0 ? 16 : 32, esz = dtype == 0 ? 4 : 2;
  MI355_REQUIRE(!x1 || (cin % CH == 0 && cin1 % CH == 0), -2, "conv2d: a two-source conv needs both channel counts to be multiples of the 64-byte chunk");
  const int cpad = (cin + CH - 1) / CH * CH;
  const int ctot = cin + cin1, ctot_pad = cpad + cin1;
  ConvDesc d; d.dtype = dtype; d.N = batch; d.Hs = h; d.Ws = w; d.C0 = cpad; d.C1 = cin1; d.ks = ksize; d.Cout = cout;
  d.knobs = &K; d.wsplit = wsplit;
  if (!x1 && cin <= 8) d.cin_real = cin;   // the padding channels pack_nhwc adds are zero: conv3x3_in_kernel contracts over the first slot only
  const bool pool = resample == 3;   // 2x2 average pool of the (normalised) input: a pre-pass, then a plain conv
  MI355_REQUIRE(!(pool && x1), -4, "conv2d: pooling over a channel concat is not supported");
  if (pool) { d.Hs = h / 2; d.Ws = w / 2; }
  d.mode = stride == 2 ? CONV_STRIDE2 : (resample == 2 ? CONV_UP2 : CONV_UNIT);
  const ConvGeom g = conv_geometry(d);
  const bool nhwc = cout % 32 == 0;
  MI355_REQUIRE(nhwc || (!emb && !res), -4, "conv2d: emb / residual epilogues need an NHWC output (cout % 32 == 0)");
  const int Hr = res_mode == RES_UP2 ? g.Ho / 2 : g.Ho, Wr = res_mode == RES_UP2 ? g.Wo / 2 : g.Wo;
  char* p = reinterpret_cast<char*>(workspace);
  char* end = p + workspace_bytes;
  void* xin = p; p += al256((size_t)batch * h * w * cpad * esz);
  void* xin1 = p; if (x1) p += al256((size_t)batch * h * w * cin1 * esz);
  void* wdev = p; const size_t wbytes = conv_packed_weight_bytes(dtype, cout, ctot, ksize, wsplit); p += al256(wbytes);
  // an up-sampling 3x3 conv may run in phase form (conv_pp bit 6): the collapsed weight image next to the nine-tap one, as the plan builder keeps both
  const bool want_up2 = d.mode == CONV_UP2 && ksize == 3 && !wsplit && (K.conv_pp & 64) && cpad == cin;
  const size_t wbytes_up2 = want_up2 ? conv_packed_weight_bytes_up2(dtype, cout, ctot) : 0;
  ExScratch xs_up2;
  void* wdev_up2 = want_up2 ? xs_up2.get(wbytes_up2) : nullptr;
  MI355_REQUIRE(!want_up2 || wdev_up2, -2, "conv2d: out of device memory");
  float* bdev = reinterpret_cast<float*>(p); p += al256((size_t)cout * 4);
  float* ga = reinterpret_cast<float*>(p); p += al256((size_t)batch * ctot_pad * 4);
  float* gb = reinterpret_cast<float*>(p); p += al256((size_t)batch * ctot_pad * 4);
  void* yout = p; p += al256((size_t)batch * g.Ho * g.Wo * cout * esz);
  void* rin = p; if (res) p += al256((size_t)batch * Hr * Wr * cout * esz);
  void* xpool = p; if (pool) p += al256((size_t)batch * (h / 2) * (w / 2) * cpad * esz);
  uint32_t* errw = reinterpret_cast<uint32_t*>(p); p += 256;
  MI355_REQUIRE(p <= end, -2, "conv2d: workspace too small");
  MI355_CHECK_HIP(hipMemsetAsync(errw, 0, 256, s));
  d.err = errw;
  int rc;
  if ((rc = pack_nhwc_launch(dtype, x, cin, nullptr, 0, batch, h * w, cpad, xin, s))) return rc;
  if (x1 && (rc = pack_nhwc_launch(dtype, x1, cin1, nullptr, 0, batch, h * w, cin1, xin1, s))) return rc;
  if (res && (rc = pack_nhwc_launch(dtype, res, cout, nullptr, 0, batch, Hr * Wr, cout, rin, s))) return rc;
  std::vector<char> packed(wbytes);
  conv_pack_weights(dtype, w_host, cout, ctot, ksize, packed.data(), wsplit);
  MI355_CHECK_HIP(hipMemcpyAsync(wdev, packed.data(), wbytes, hipMemcpyHostToDevice, s));
  std::vector<char> packed_up2(wbytes_up2);
  if (want_up2) {
    conv_pack_weights_up2(dtype, w_host, cout, ctot, packed_up2.data());
    MI355_CHECK_HIP(hipMemcpyAsync(wdev_up2, packed_up2.data(), wbytes_up2, hipMemcpyHostToDevice, s));
    d.w_up2 = wdev_up2;
  }
  if (bias_host) MI355_CHECK_HIP(hipMemcpyAsync(bdev, bias_host, (size_t)cout * 4, hipMemcpyHostToDevice, s));
  if (gn_gamma) {
    MI355_REQUIRE(ctot % 32 == 0 && cin % 32 == 0, -2, "conv2d: the GroupNorm32 prologue needs channels % 32 == 0");
    GnDesc gd; gd.dtype = dtype; gd.src0 = xin; gd.C0 = cpad; gd.src1 = x1 ? xin1 : nullptr; gd.C1 = cin1; gd.N = batch; gd.HW = h * w;
    gd.gamma = gn_gamma; gd.beta = gn_beta;
    gd.a = ga; gd.b = gb;
    if ((rc = gn_affine_launch(gd, s))) return rc;
    if (!pool) { d.pro_a = ga; d.pro_b = gb; d.pro_silu = gn_silu; }
  }
  if (x1) d.src1 = xin1;
  if (emb) { d.emb = emb; d.emb_stride = cout; }
  if (res) { d.res = rin; d.res_mode = res_mode; }
  d.src0 = xin;
  if (pool) {
    if ((rc = affine_pool_launch(dtype, xin, gn_gamma ? ga : nullptr, gn_gamma ? gb : nullptr, gn_silu, xpool, batch, h, w, cpad, s))) return rc;
    d.src0 = xpool;
  } d.w = wdev; d.bias = bias_host ? bdev : nullptr;
  d.out_mode = nhwc ? OUT_NHWC : OUT_NCHW_F32;
  d.out = nhwc ? yout : (void*)y;
#ifdef CONV_STAMPS
  const size_t nwaves = (size_t)g.grid_m * g.grid_n * 4;
  MI355_REQUIRE(p + 65536 + nwaves * 64 <= end, -2, "conv2d: workspace too small (stamps)");
  MI355_CHECK_HIP(hipMemsetAsync(p, 0, 65536 + nwaves * 64, s));
  unsigned long long* clk = reinterpret_cast<unsigned long long*>(p);   // [4096 waves][shader cycles, 100-MHz ticks]: CLK_FLUSH
  p += 65536;
  d.dbg = p;
#endif
  // ---- extras (mi355_conv2d_ex): the small-level kernel's fused forms, as the engine's walker asks for them ----
  ExScratch xs;
  bool ex_stats = false;
  void* act_dev[2] = {nullptr, nullptr};
  std::vector<char> packed_f; std::vector<float> bias_f;
  if (ex) {
    ex->act_done = 0; ex->skip_done = 0;
    ex_stats = ex->route[3] == MI355_CONV_EXTRAS_STATS && ex->stat_a;   // the struct's later tail is read only behind this word
    if (ex_stats) ex->stat_slots = 0;
    for (int i = 0; i < 4; ++i) ex->route[i] = -1;
    MI355_REQUIRE(nhwc && !pool, -4, "conv2d_ex: extras need an NHWC output and no pooling");
    if (ex->skip_x0) {
      MI355_REQUIRE(ksize == 3 && stride == 1 && !resample && !x1 && !res && !wsplit && ex->skip_w_host && ex->skip_c0 > 0, -1, "conv2d_ex: the fused skip conv goes with a plain 3x3 conv of one source");
      MI355_REQUIRE((ex->skip_x1 != nullptr) == (ex->skip_c1 > 0), -1, "conv2d_ex: skip_x1 and skip_c1 go together");
      const int cs = ex->skip_c0 + ex->skip_c1;
      void* k0 = xs.get((size_t)batch * h * w * ex->skip_c0 * esz);
      void* k1 = ex->skip_x1 ? xs.get((size_t)batch * h * w * ex->skip_c1 * esz) : nullptr;
      const size_t fb = conv_packed_weight_bytes_skip(dtype, cout, ctot, cs);
      void* wf = xs.get(fb);
      MI355_REQUIRE(k0 && wf && (!ex->skip_x1 || k1), -2, "conv2d_ex: out of device memory");
      if ((rc = pack_nhwc_launch(dtype, ex->skip_x0, ex->skip_c0, nullptr, 0, batch, h * w, ex->skip_c0, k0, s))) return rc;
      if (k1 && (rc = pack_nhwc_launch(dtype, ex->skip_x1, ex->skip_c1, nullptr, 0, batch, h * w, ex->skip_c1, k1, s))) return rc;
      packed_f.resize(fb);
      conv_pack_weights_skip(dtype, w_host, ex->skip_w_host, cout, ctot, cs, packed_f.data());
      MI355_CHECK_HIP(hipMemcpyAsync(wf, packed_f.data(), fb, hipMemcpyHostToDevice, s));
      bias_f.assign((size_t)cout, 0.f);
      for (int i = 0; i < cout; ++i) bias_f[i] = (bias_host ? bias_host[i] : 0.f) + (ex->skip_bias_host ? ex->skip_bias_host[i] : 0.f);
      MI355_CHECK_HIP(hipMemcpyAsync(bdev, bias_f.data(), (size_t)cout * 4, hipMemcpyHostToDevice, s));
      d.w = wf; d.bias = bdev;
      d.skip_src0 = k0; d.skip_C0 = ex->skip_c0; d.skip_src1 = k1; d.skip_C1 = ex->skip_c1;
    }
    for (int k = 0; k < 2; ++k) {
      if (!ex->act_out[k]) continue;
      MI355_REQUIRE(k == 0 || ex->act_out[0], -1, "conv2d_ex: site 1 without site 0");
      MI355_REQUIRE(ex->act_gamma[k] && ex->act_beta[k] && ex->act_ctotal[k] % 32 == 0 && ex->act_coff[k] >= 0 && ex->act_coff[k] + cout <= ex->act_ctotal[k], -1, "conv2d_ex: bad GroupNorm site");
      const size_t ab = (size_t)batch * g.Ho * g.Wo * ex->act_ctotal[k] * esz;
      act_dev[k] = xs.get(ab);
      MI355_REQUIRE(act_dev[k], -2, "conv2d_ex: out of device memory");
      MI355_CHECK_HIP(hipMemsetAsync(act_dev[k], 0, ab, s));
    }
    if (act_dev[0]) {
      d.act_out = act_dev[0]; d.act_gamma = ex->act_gamma[0] + ex->act_coff[0]; d.act_beta = ex->act_beta[0] + ex->act_coff[0];
      d.act_silu = ex->act_silu[0]; d.act_stride = ex->act_ctotal[0]; d.act_coff = ex->act_coff[0]; d.act_cpg = ex->act_ctotal[0] / 32; d.act_raw = 1;
      if (ex->act_film) { d.act_film = ex->act_film; d.act_film_stride = 2 * cout; }
    }
    if (act_dev[1]) {
      d.act2_out = act_dev[1]; d.act2_gamma = ex->act_gamma[1] + ex->act_coff[1]; d.act2_beta = ex->act_beta[1] + ex->act_coff[1];
      d.act2_silu = ex->act_silu[1]; d.act2_stride = ex->act_ctotal[1]; d.act2_coff = ex->act_coff[1]; d.act2_cpg = ex->act_ctotal[1] / 32;
    }
  }
  if (ex_stats) {   // the output's GroupNorm partial sums (a slot no wave writes stays NaN)
    MI355_REQUIRE(nhwc && ex->stat_b && ex->stat_gamma && ex->stat_beta, -1, "conv2d_ex: statistics need an NHWC output, stat_b, stat_gamma and stat_beta");
    const int cap = 4 * ((g.Ho * g.Wo + 63) / 64) + 8;   // the plan builder's stats_cap (unet_engine.hip)
    const size_t sb = (size_t)batch * cap * (cout / 4) * 2 * 4;
    float* st = reinterpret_cast<float*>(xs.get(sb));
    MI355_REQUIRE(st, -2, "conv2d_ex: out of device memory");
    MI355_CHECK_HIP(hipMemsetAsync(st, 0xFF, sb, s));
    d.gn_stats = st; d.gn_slots_cap = cap;
  }
  ConvRoute route;
  if ((rc = conv_route(d, &route))) {
    if (d.skip_src0) { mi355_set_error("conv2d_ex: this launch cannot carry the fused skip conv (shape, batch or knobs)"); return MI355_ERR_UNSUPPORTED; }
    return rc;
  }
  if ((rc = conv_launch(d, route, s))) return rc;
  if (ex) {
    ex->skip_done = route.skip; ex->act_done = route.act_done;
    if (ex_stats && route.gn_slots > 0) {
      GnFinDesc f; f.stats0 = d.gn_stats; f.slots0 = route.gn_slots; f.C0 = cout;
      f.N = batch; f.HW = g.Ho * g.Wo; f.gamma = ex->stat_gamma; f.beta = ex->stat_beta;
      f.a = ex->stat_a; f.b = ex->stat_b; f.dtype = dtype; f.src0 = yout;
      if ((rc = gn_finalize_launch(f, s))) return rc;
      ex->stat_slots = route.gn_slots;
    }
    ex->route[0] = route.kernel; ex->route[1] = route.form; ex->route[2] = route.geom.BM; ex->route[3] = route.geom.BN;
    for (int k = 0; k < 2; ++k)
      if (act_dev[k] && (route.act_done & (1 << k)) && (rc = unpack_nchw_launch(dtype, act_dev[k], batch, g.Ho * g.Wo, ex->act_ctotal[k], ex->act_out[k], s))) return rc;
  }
  if (K.conv_time_reps > 0) {   // diagnostic: average duration of the conv launch alone
    const int reps = K.conv_time_reps;
    hipEvent_t e0, e1;
    MI355_CHECK_HIP(hipEventCreate(&e0)); MI355_CHECK_HIP(hipEventCreate(&e1));
    MI355_CHECK_HIP(hipEventRecord(e0, s));
    ConvRoute plain = route; plain.act_done = 0;   // the same kernel without the fused GroupNorm sites
    for (int i = 0; i < reps; ++i) if ((rc = conv_launch(d, plain, s))) return rc;
    MI355_CHECK_HIP(hipEventRecord(e1, s));
    MI355_CHECK_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    MI355_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
    const double us = 1e3 * ms / reps, fl = 2.0 * batch * g.Ho * g.Wo * (double)cout * ctot * ksize * ksize;
    fprintf(stderr, "[conv time] %d launches, %.1f us each, %.0f TFLOP/s\n", reps, us, fl / us * 1e-6);
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  }
  if (nhwc && (rc = unpack_nchw_launch(dtype, yout, batch, g.Ho * g.Wo, cout, y, s))) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));  // `packed` is a temporary host buffer
  {
    uint32_t ev = 0;
    MI355_CHECK_HIP(hipMemcpy(&ev, errw, 4, hipMemcpyDeviceToHost));
    if (ev) { mi355_set_error("conv2d: the persistent kernel gave up a bounded counter wait (hand-over stalled): the output is invalid"); return MI355_ERR_TIMEOUT; }
  }
#ifdef CONV_STAMPS
  {
    std::vector<unsigned long long> hv(nwaves * 8);
    MI355_CHECK_HIP(hipMemcpy(hv.data(), p, nwaves * 64, hipMemcpyDeviceToHost));
    static const char* names_plain[8] = {"setup", "commit_patch", "barrier_A", "commit_w(+vmcnt)", "barrier_B", "prefetch_issue", "mma", "epilogue"};
    // warp-specialised kernel: slots 0-4 are written by loader waves only, 5-7 by consumer waves only (half the waves each)
    static const char* names_ws[8] = {"L:fill", "L:commit_w", "L:commit_frag", "L:issue", "L:barrier", "C:barrier", "C:mma_row", "C:epilogue+setup"};
    const bool ws_names = K.conv_ws != 0;
    const char** names = ws_names ? names_ws : names_plain;
    double h[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tot = 0;
    for (size_t w = 0; w < nwaves; ++w) for (int k = 0; k < 8; ++k) h[k] += (double)hv[w * 8 + k];
    for (int k = 0; k < 8; ++k) tot += h[k];
    {   // in-kernel clock of the LAST launch (after conv_time_reps back-to-back launches: the sustained clock), median over waves
      std::vector<unsigned long long> hc(8192);
      MI355_CHECK_HIP(hipMemcpy(hc.data(), clk, 65536, hipMemcpyDeviceToHost));
      std::vector<double> mhz;
      for (size_t w = 0; w < 4096; ++w) if (hc[2 * w + 1] > 0) mhz.push_back(100.0 * (double)hc[2 * w] / (double)hc[2 * w + 1]);
      if (!mhz.empty()) {
        std::sort(mhz.begin(), mhz.end());
        fprintf(stderr, "[conv clock] %zu waves: in-kernel clock min %.0f median %.0f max %.0f MHz\n", mhz.size(), mhz.front(), mhz[mhz.size() / 2], mhz.back());
      }
    }
    if (g.BM == 256 && g.BN == 256 && nwaves * 8 >= 2048 * 8 + 160) {   // timeline of workgroup 0, taps 8 .. 11 (PP_TRACE): cycles relative to wave 0's first stamp
      const unsigned long long* tr = hv.data() + 2048 * 8;
      const unsigned long long t0 = tr[0];
      static const char* ev[5] = {"issued", "vmcnt", "barL", "mfma", "barM"};
      for (int w = 0; w < 8; ++w) {
        fprintf(stderr, "[pp trace] wave %d:", w);
        for (int i = 0; i < 20; ++i) fprintf(stderr, " %s%d=%lld", ev[i % 5], 8 + i / 5, (long long)(int32_t)(uint32_t)(tr[w * 20 + i] - t0));
        fprintf(stderr, "\n");
      }
    }
    if (g.BM == 256 && g.BN == 256) {   // ping-pong kernel (conv_pp.inc.h): 8 waves per workgroup, waves 0-3 = group 0, 4-7 = group 1 (one tick behind)
      static const char* names_pp[8] = {"L:reads+dma", "L:vmcnt", "L:barrier", "M:mfma", "M:barrier", "E:epilogue", "E:rejoin", "tile_head"};
      for (int grp = 0; grp < 2; ++grp) {
        double hp[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tp = 0; size_t nw = 0;
        for (size_t w = 0; w < nwaves; ++w) {
          if (((w >> 2) & 1) != (size_t)grp) continue;
          double tw = 0;
          for (int k = 0; k < 8; ++k) tw += (double)hv[w * 8 + k];
          if (tw == 0) continue;
          ++nw;
          for (int k = 0; k < 8; ++k) hp[k] += (double)hv[w * 8 + k];
          tp += tw;
        }
        if (!nw) continue;
        fprintf(stderr, "[conv stamps] ping-pong group %d, waves %zu, cycles/wave %.0f:", grp, nw, tp / nw);
        for (int k = 0; k < 8; ++k) fprintf(stderr, " %s %.0f (%.1f%%)", names_pp[k], hp[k] / nw, 100.0 * hp[k] / tp);
        fprintf(stderr, "\n");
      }
    } else if (tot > 0) {
      fprintf(stderr, "[conv stamps] waves %zu, cycles/wave %.0f:", nwaves, tot / nwaves);
      for (int k = 0; k < 8; ++k) fprintf(stderr, " %s %.0f (%.1f%%)", names[k], h[k] / nwaves, 100.0 * h[k] / tot);
      fprintf(stderr, "\n");
    }
  }
#endif
  return 0;
}

int mi355_qkv_attention(const float* qkv, float* out, int batch, int heads, int head_channels, int length, int new_order, int dtype,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(qkv && out && workspace, -1, "qkv_attention: null argument");
  hipStream_t s = S(stream);
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16 || dtype == MI355_F16, -1, "qkv_attention: bad dtype");
  dtype = dtype == MI355_F16 ? DT_F16 : dtype;
  const int esz = dtype == 0 ? 4 : 2, C = heads * head_channels;
  char* p = reinterpret_cast<char*>(workspace);
  void* qin = p; p += al256((size_t)batch * length * 3 * C * esz);
  void* o = p; p += al256((size_t)batch * length * C * esz);
  MI355_REQUIRE(p <= reinterpret_cast<char*>(workspace) + workspace_bytes, -2, "qkv_attention: workspace too small");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, qkv, 3 * C, nullptr, 0, batch, length, 3 * C, qin, s))) return rc;
  AttnDesc a; a.dtype = dtype; a.qkv = qin; a.out = o; a.N = batch; a.T = length; a.heads = heads; a.ch = head_channels; a.new_order = new_order;
  if ((rc = attention_launch(a, s))) return rc;
  return unpack_nchw_launch(dtype, o, batch, length, C, out, s);
}

int mi355_qkv_attention_vjp(const float* qkv, const float* grad_out, float* grad_qkv, int batch, int heads, int head_channels, int length,
                            int new_order, int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(qkv && grad_out && grad_qkv && workspace, -1, "qkv_attention_vjp: null argument");
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16, -1, "qkv_attention_vjp: dtype must be MI355_F32 or MI355_BF16 (the attention backward has no other form)");
  MI355_REQUIRE(batch > 0 && heads > 0 && head_channels > 0 && length > 0, -1, "qkv_attention_vjp: bad sizes");
  hipStream_t s = S(stream);
  const int esz = dtype == DT_F32 ? 4 : 2, C = heads * head_channels;
  const size_t rows = (size_t)batch * length;
  char* p = reinterpret_cast<char*>(workspace);
  void* qin = p; p += al256(rows * 3 * C * esz);
  void* din = p; p += al256(rows * C * esz);
  void* a = p; p += al256(rows * C * esz);
  void* dq = p; p += al256(rows * 3 * C * esz);
  float* Ls = reinterpret_cast<float*>(p); p += al256((size_t)batch * heads * length * 4);
  float* Ds = reinterpret_cast<float*>(p); p += al256((size_t)batch * heads * length * 4);
  MI355_REQUIRE(p <= reinterpret_cast<char*>(workspace) + workspace_bytes, -2, "qkv_attention_vjp: workspace too small");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, qkv, 3 * C, nullptr, 0, batch, length, 3 * C, qin, s))) return rc;
  if ((rc = pack_nhwc_launch(dtype, grad_out, C, nullptr, 0, batch, length, C, din, s))) return rc;
  // A from the forward kernel a differentiable plan runs (OP_ATTN), then the two backward kernels as unet_backward calls them
  AttnDesc f; f.dtype = dtype; f.qkv = qin; f.out = a; f.N = batch; f.T = length; f.heads = heads; f.ch = head_channels; f.new_order = new_order;
  if ((rc = attention_launch(f, s))) return rc;
  AttnBwdDesc b; b.dtype = dtype; b.qkv = qin; b.a = a; b.da = din; b.dqkv = dq; b.L = Ls; b.D = Ds;
  b.N = batch; b.T = length; b.heads = heads; b.ch = head_channels; b.new_order = new_order;
  if ((rc = attention_bwd_launch(b, s))) return rc;
  return unpack_nchw_launch(dtype, dq, batch, length, 3 * C, grad_qkv, s);
}

// ---- the fused AttentionBlock front half (ABI 108): attn_fused_launch as the engine calls it, (a, b) given instead of derived ------
int mi355_attn_block_fused(const float* x, const float* a, const float* b, const float* w_host, const float* bias_host, float* out, int batch,
                           int channels, int length, int heads, int new_order, int dtype, const mi355_debug_config* debug, int32_t form[3],
                           void* workspace, int64_t workspace_bytes, void* stream) {
  if (form) form[0] = form[1] = form[2] = -1;
  MI355_REQUIRE(x && a && b && w_host && bias_host && out && workspace, -1, "attn_block_fused: null argument");
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16 || dtype == MI355_F16, -1, "attn_block_fused: dtype must be MI355_F32, MI355_BF16 or MI355_F16");
  MI355_REQUIRE(batch > 0 && channels > 0 && length > 0 && heads > 0, -1, "attn_block_fused: bad sizes");
  dtype = dtype == MI355_F16 ? DT_F16 : dtype;
  hipStream_t s = S(stream);
  const int C = channels;
  AttnFusedDesc d; d.dtype = dtype; d.N = batch; d.T = length; d.C = C; d.heads = heads; d.ch = C / heads; d.new_order = new_order;
  d.knobs = debug; d.form = form;
  // a shape the fused kernels do not take is the launcher's own refusal, before anything is enqueued
  if (!attn_fused_eligible(d.dtype, d.T, d.C, d.heads, d.ch, d.knobs)) return attn_fused_launch(d, s);
  const size_t esz = dtype == DT_F32 ? 4 : 2;
  const size_t wbytes = conv_packed_weight_bytes(dtype, 3 * C, C, 1, 0);
  char* p = reinterpret_cast<char*>(workspace);
  void* xin = p; p += al256((size_t)batch * length * C * esz);
  void* o = p; p += al256((size_t)batch * length * C * esz);
  void* wdev = p; p += al256(wbytes);
  float* bdev = reinterpret_cast<float*>(p); p += al256((size_t)3 * C * 4);
  MI355_REQUIRE(p <= reinterpret_cast<char*>(workspace) + workspace_bytes, -2, "attn_block_fused: workspace too small");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, x, C, nullptr, 0, batch, length, C, xin, s))) return rc;
  std::vector<char> packed(wbytes);
  conv_pack_weights(dtype, w_host, 3 * C, C, 1, packed.data(), 0);
  MI355_CHECK_HIP(hipMemcpyAsync(wdev, packed.data(), wbytes, hipMemcpyHostToDevice, s));
  MI355_CHECK_HIP(hipMemcpyAsync(bdev, bias_host, (size_t)3 * C * 4, hipMemcpyHostToDevice, s));
  MI355_CHECK_HIP(hipMemsetAsync(o, 0xFF, (size_t)batch * length * C * esz, s));   // NaN in every element type until the kernel writes it
  d.x = xin; d.ga = a; d.gb = b; d.w = wdev; d.bias = bdev; d.out = o;
  if ((rc = attn_fused_launch(d, s))) return rc;
  if ((rc = unpack_nchw_launch(dtype, o, batch, length, C, out, s))) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));   // `packed` is a temporary host buffer
  return 0;
}

// ---- GroupNorm test ops (ABI 107): the kernels the network launches, one op each, NCHW fp32 at the boundary ------------------------
// Device scratch is the op's own (ExScratch); every op synchronises the stream before it returns.
namespace {
int gn_op_dtype(int dtype, bool backward, const char* who, int* out) {
  if (backward) {
    if (dtype != MI355_F32 && dtype != MI355_BF16) { mi355_set_error(std::string(who) + ": dtype must be MI355_F32 or MI355_BF16 (the backward kernels have no other form)"); return -1; }
  } else if (dtype != MI355_F32 && dtype != MI355_BF16 && dtype != MI355_F16) { mi355_set_error(std::string(who) + ": dtype must be MI355_F32, MI355_BF16 or MI355_F16"); return -1; }
  *out = dtype == MI355_F16 ? DT_F16 : dtype;
  return 0;
}
}  // namespace

int mi355_gn_affine(const float* x, const float* x1, const float* gamma, const float* beta, const float* film, float eps, float* a, float* b,
                    float* mean, float* rstd, float* y, int y_silu, int32_t* form, int batch, int c0, int c1, int hw, int dtype, void* stream) {
  MI355_REQUIRE(x && gamma && beta && a && b && batch > 0 && c0 > 0 && c1 >= 0 && hw > 0, -1, "gn_affine: bad argument");
  MI355_REQUIRE((x1 != nullptr) == (c1 > 0) && (mean != nullptr) == (rstd != nullptr), -1, "gn_affine: x1 / c1 and mean / rstd go together");
  if (int rc = gn_op_dtype(dtype, false, "gn_affine", &dtype)) return rc;
  hipStream_t s = S(stream);
  const size_t esz = dtype == 0 ? 4 : 2;
  const int C = c0 + c1;
  ExScratch xs;
  void* p0 = xs.get((size_t)batch * hw * c0 * esz);
  void* p1 = x1 ? xs.get((size_t)batch * hw * c1 * esz) : nullptr;
  void* py = y ? xs.get((size_t)batch * hw * C * esz) : nullptr;
  MI355_REQUIRE(p0 && (!x1 || p1) && (!y || py), -2, "gn_affine: out of device memory");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, x, c0, nullptr, 0, batch, hw, c0, p0, s))) return rc;
  if (x1 && (rc = pack_nhwc_launch(dtype, x1, c1, nullptr, 0, batch, hw, c1, p1, s))) return rc;
  if (py) MI355_CHECK_HIP(hipMemsetAsync(py, 0xFF, (size_t)batch * hw * C * esz, s));   // NaN in every element type until the kernel writes it
  GnDesc g; g.dtype = dtype; g.src0 = p0; g.C0 = c0; g.src1 = p1; g.C1 = c1; g.N = batch; g.HW = hw; g.eps = eps;
  g.gamma = gamma; g.beta = beta; g.film = film; g.film_stride = film ? 2 * C : 0;
  g.a = a; g.b = b; g.mean = mean; g.rstd = rstd; g.y = py; g.y_silu = y_silu;
  if (form) *form = gn_affine_form(g);
  if ((rc = gn_affine_launch(g, s))) return rc;
  if (py && (rc = unpack_nchw_launch(dtype, py, batch, hw, C, y, s))) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int mi355_conv2d_gn(const float* x0, const float* w0_host, const float* bias0_host, float* y0, int cin0, int cout0, const float* x1,
                    const float* w1_host, const float* bias1_host, float* y1, int cin1, int cout1, int batch, int h, int w, int ksize, int stride,
                    int resample, const float* gamma, const float* beta, const float* film, float eps, float* a, float* b, int dtype,
                    const mi355_debug_config* debug, int32_t info[6], void* stream) {
  const mi355_debug_config& K = debug ? *debug : mi355_default_debug();
  MI355_REQUIRE(x0 && w0_host && y0 && gamma && beta && a && b && info && batch > 0, -1, "conv2d_gn: bad argument");
  MI355_REQUIRE((x1 != nullptr) == (cout1 > 0) && (!x1 || (w1_host && y1 && cin1 > 0)), -1, "conv2d_gn: the second producer needs x1, w1, y1, cin1 and cout1");
  MI355_REQUIRE((stride == 1 || stride == 2) && (resample == 0 || resample == 2) && !(stride == 2 && resample), -1, "conv2d_gn: stride 1 or 2, resample 0 or 2 (nearest x2)");
  if (int rc = gn_op_dtype(dtype, false, "conv2d_gn", &dtype)) return rc;
  hipStream_t s = S(stream);
  const int CH = dtype == 0 ? 16 : 32;
  const size_t esz = dtype == 0 ? 4 : 2;
  ExScratch xs;
  const float* xin[2] = {x0, x1}; const float* wh[2] = {w0_host, w1_host}; const float* bh[2] = {bias0_host, bias1_host};
  float* yo[2] = {y0, y1}; const int cin[2] = {cin0, cin1}, cout[2] = {cout0, cout1};
  void* out_dev[2] = {nullptr, nullptr}; float* st[2] = {nullptr, nullptr};
  int Ho = 0, Wo = 0, rc;
  for (int i = 0; i < 6; ++i) info[i] = 0;
  std::vector<char> packed[2], packed_up2[2];
  for (int k = 0; k < (x1 ? 2 : 1); ++k) {
    MI355_REQUIRE(cout[k] % 32 == 0, -2, "conv2d_gn: NHWC outputs need cout % 32 == 0");
    const int cpad = (cin[k] + CH - 1) / CH * CH;
    ConvDesc d; d.dtype = dtype; d.N = batch; d.Hs = h; d.Ws = w; d.C0 = cpad; d.ks = ksize; d.Cout = cout[k]; d.knobs = &K;
    d.mode = stride == 2 ? CONV_STRIDE2 : (resample == 2 ? CONV_UP2 : CONV_UNIT);
    if (cin[k] <= 8) d.cin_real = cin[k];
    const ConvGeom g = conv_geometry(d);
    MI355_REQUIRE(k == 0 || (g.Ho == Ho && g.Wo == Wo), -2, "conv2d_gn: the producers' outputs differ in size");
    Ho = g.Ho; Wo = g.Wo;
    void* xd = xs.get((size_t)batch * h * w * cpad * esz);
    const size_t wbytes = conv_packed_weight_bytes(dtype, cout[k], cin[k], ksize, 0);
    void* wd = xs.get(wbytes);
    float* bd = reinterpret_cast<float*>(xs.get((size_t)cout[k] * 4));
    out_dev[k] = xs.get((size_t)batch * Ho * Wo * cout[k] * esz);
    const int cap = 4 * ((Ho * Wo + 63) / 64) + 8;   // the plan builder's stats_cap (unet_engine.hip)
    st[k] = reinterpret_cast<float*>(xs.get((size_t)batch * cap * (cout[k] / 4) * 2 * 4));
    uint32_t* errw = reinterpret_cast<uint32_t*>(xs.get(256));
    MI355_REQUIRE(xd && wd && bd && out_dev[k] && st[k] && errw, -2, "conv2d_gn: out of device memory");
    MI355_CHECK_HIP(hipMemsetAsync(errw, 0, 256, s));
    MI355_CHECK_HIP(hipMemsetAsync(st[k], 0xFF, (size_t)batch * cap * (cout[k] / 4) * 2 * 4, s));   // a slot no wave writes stays NaN
    if ((rc = pack_nhwc_launch(dtype, xin[k], cin[k], nullptr, 0, batch, h * w, cpad, xd, s))) return rc;
    packed[k].resize(wbytes);
    conv_pack_weights(dtype, wh[k], cout[k], cin[k], ksize, packed[k].data(), 0);
    MI355_CHECK_HIP(hipMemcpyAsync(wd, packed[k].data(), wbytes, hipMemcpyHostToDevice, s));
    if (d.mode == CONV_UP2 && ksize == 3 && (K.conv_pp & 64) && cpad == cin[k]) {   // the phase form's collapsed image too (the route decides)
      const size_t ub = conv_packed_weight_bytes_up2(dtype, cout[k], cin[k]);
      void* wu = xs.get(ub);
      MI355_REQUIRE(wu, -2, "conv2d_gn: out of device memory");
      packed_up2[k].resize(ub);
      conv_pack_weights_up2(dtype, wh[k], cout[k], cin[k], packed_up2[k].data());
      MI355_CHECK_HIP(hipMemcpyAsync(wu, packed_up2[k].data(), ub, hipMemcpyHostToDevice, s));
      d.w_up2 = wu;
    }
    if (bh[k]) MI355_CHECK_HIP(hipMemcpyAsync(bd, bh[k], (size_t)cout[k] * 4, hipMemcpyHostToDevice, s));
    d.src0 = xd; d.w = wd; d.bias = bh[k] ? bd : nullptr; d.out = out_dev[k]; d.out_mode = OUT_NHWC; d.err = errw;
    d.gn_stats = st[k]; d.gn_slots_cap = cap;
    ConvRoute route;
    if ((rc = conv_route(d, &route)) || (rc = conv_launch(d, route, s))) return rc;
    info[3 * k] = route.kernel; info[3 * k + 1] = route.gn_slots; info[3 * k + 2] = route.form;
    if ((rc = unpack_nchw_launch(dtype, out_dev[k], batch, Ho * Wo, cout[k], yo[k], s))) return rc;
    MI355_CHECK_HIP(hipStreamSynchronize(s));   // the packed weights are staged from host memory
    uint32_t ev = 0;
    MI355_CHECK_HIP(hipMemcpy(&ev, errw, 4, hipMemcpyDeviceToHost));
    if (ev) { mi355_set_error("conv2d_gn: the persistent kernel gave up a bounded counter wait: the output is invalid"); return MI355_ERR_TIMEOUT; }
  }
  if (info[1] > 0 && (!x1 || info[4] > 0)) {
    GnFinDesc f; f.stats0 = st[0]; f.slots0 = info[1]; f.C0 = cout0;
    if (x1) { f.stats1 = st[1]; f.slots1 = info[4]; f.C1 = cout1; }
    f.N = batch; f.HW = Ho * Wo; f.eps = eps; f.gamma = gamma; f.beta = beta; f.film = film; f.film_stride = film ? 2 * (cout0 + cout1) : 0;
    f.a = a; f.b = b; f.dtype = dtype; f.src0 = out_dev[0]; f.src1 = out_dev[1];
    if ((rc = gn_finalize_launch(f, s))) return rc;
  }
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int mi355_affine_pool(const float* x, const float* a, const float* b, int silu, float* out, int batch, int channels, int h, int w, int dtype,
                      void* stream) {
  MI355_REQUIRE(x && out && (a != nullptr) == (b != nullptr) && batch > 0 && channels > 0 && h > 0 && w > 0, -1, "affine_pool: bad argument");
  if (int rc = gn_op_dtype(dtype, false, "affine_pool", &dtype)) return rc;
  hipStream_t s = S(stream);
  const size_t esz = dtype == 0 ? 4 : 2;
  ExScratch xs;
  void* pi = xs.get((size_t)batch * h * w * channels * esz);
  void* po = xs.get((size_t)batch * (h / 2) * (w / 2) * channels * esz);
  MI355_REQUIRE(pi && po, -2, "affine_pool: out of device memory");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, x, channels, nullptr, 0, batch, h * w, channels, pi, s))) return rc;
  MI355_CHECK_HIP(hipMemsetAsync(po, 0xFF, (size_t)batch * (h / 2) * (w / 2) * channels * esz, s));
  if ((rc = affine_pool_launch(dtype, pi, a, b, silu, po, batch, h, w, channels, s))) return rc;
  if ((rc = unpack_nchw_launch(dtype, po, batch, (h / 2) * (w / 2), channels, out, s))) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int mi355_gn_silu_vjp(const float* x0, const float* x1, const float* gamma, const float* beta, const float* film, float eps, int silu,
                      const float* du, int du_stride, float* g0, float* g1, int acc0, int acc1, int batch, int c0, int c1, int hw, int dtype,
                      void* stream) {
  MI355_REQUIRE(x0 && gamma && beta && du && g0 && batch > 0 && c0 > 0 && c1 >= 0 && hw > 0, -1, "gn_silu_vjp: bad argument");
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16, -1, "gn_silu_vjp: dtype must be MI355_F32 or MI355_BF16 (the GroupNorm backward has no other form)");
  MI355_REQUIRE((x1 != nullptr) == (c1 > 0) && (x1 != nullptr) == (g1 != nullptr), -1, "gn_silu_vjp: x1, g1 and c1 go together");
  const int C = c0 + c1;
  MI355_REQUIRE(du_stride >= C, -2, "gn_silu_vjp: du_stride must be at least c0 + c1");
  hipStream_t s = S(stream);
  const size_t esz = dtype == 0 ? 4 : 2;
  ExScratch xs;
  void* p0 = xs.get((size_t)batch * hw * c0 * esz);
  void* p1 = x1 ? xs.get((size_t)batch * hw * c1 * esz) : nullptr;
  void* pd = xs.get((size_t)batch * hw * du_stride * esz);
  void* q0 = xs.get((size_t)batch * hw * c0 * esz);
  void* q1 = x1 ? xs.get((size_t)batch * hw * c1 * esz) : nullptr;
  float* ab = reinterpret_cast<float*>(xs.get(((size_t)2 * batch * C + (size_t)2 * batch * 32) * 4));
  MI355_REQUIRE(p0 && pd && q0 && ab && (!x1 || (p1 && q1)), -2, "gn_silu_vjp: out of device memory");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, x0, c0, nullptr, 0, batch, hw, c0, p0, s))) return rc;
  if (x1 && (rc = pack_nhwc_launch(dtype, x1, c1, nullptr, 0, batch, hw, c1, p1, s))) return rc;
  if ((rc = pack_nhwc_launch(dtype, du, C, nullptr, 0, batch, hw, du_stride, pd, s))) return rc;   // channels C .. du_stride: zero padding, as a channel-padded dgrad conv leaves it
  // a gradient the kernel accumulates into is the caller's, packed; one it overwrites starts as NaN
  if (acc0) { if ((rc = pack_nhwc_launch(dtype, g0, c0, nullptr, 0, batch, hw, c0, q0, s))) return rc; }
  else MI355_CHECK_HIP(hipMemsetAsync(q0, 0xFF, (size_t)batch * hw * c0 * esz, s));
  if (x1) {
    if (acc1) { if ((rc = pack_nhwc_launch(dtype, g1, c1, nullptr, 0, batch, hw, c1, q1, s))) return rc; }
    else MI355_CHECK_HIP(hipMemsetAsync(q1, 0xFF, (size_t)batch * hw * c1 * esz, s));
  }
  // forward statistics as a differentiable plan keeps them (unet_engine.hip: a, b, mean, rstd of the site), then the backward kernel
  GnDesc g; g.dtype = dtype; g.src0 = p0; g.C0 = c0; g.src1 = p1; g.C1 = c1; g.N = batch; g.HW = hw; g.eps = eps;
  g.gamma = gamma; g.beta = beta; g.film = film; g.film_stride = film ? 2 * C : 0;
  g.a = ab; g.b = ab + (size_t)batch * C; g.mean = ab + (size_t)2 * batch * C; g.rstd = g.mean + (size_t)batch * 32;
  if ((rc = gn_affine_launch(g, s))) return rc;
  GnBwdDesc d; d.dtype = dtype; d.x0 = p0; d.x1 = p1; d.C0 = c0; d.C1 = c1; d.du = pd; d.du_stride = du_stride; d.N = batch; d.HW = hw; d.silu = silu;
  d.a = g.a; d.b = g.b; d.mean = g.mean; d.rstd = g.rstd; d.g0 = q0; d.g1 = q1; d.acc0 = acc0; d.acc1 = acc1;
  if ((rc = gn_silu_bwd_launch(d, s))) return rc;
  if ((rc = unpack_nchw_launch(dtype, q0, batch, hw, c0, g0, s))) return rc;
  if (x1 && (rc = unpack_nchw_launch(dtype, q1, batch, hw, c1, g1, s))) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int mi355_grad_gather(const float* src, float* dst, int batch, int cd, int hd, int wd, int hs, int ws, int src_channels, int src_coff, int mode,
                      int accumulate, float scale, int dtype, void* stream) {
  MI355_REQUIRE(src && dst && batch > 0 && cd > 0 && hd > 0 && wd > 0 && hs > 0 && ws > 0, -1, "grad_gather: bad argument");
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16, -1, "grad_gather: dtype must be MI355_F32 or MI355_BF16 (the gather kernels have no other form)");
  MI355_REQUIRE(src_coff >= 0 && src_coff + cd <= src_channels, -2, "grad_gather: channels src_coff .. src_coff + cd must lie inside the source");
  // every source pixel the mode reads must exist (the kernel does not clamp): identity; 2x2 blocks; half-resolution; zero insertion (any source size)
  const bool fits = mode == GATHER_SAME ? (hs == hd && ws == wd) : mode == GATHER_POOL ? (hs == 2 * hd && ws == 2 * wd)
                  : mode == GATHER_UP ? (2 * hs >= hd && 2 * ws >= wd) : mode == GATHER_STUFF;
  MI355_REQUIRE(fits, -2, "grad_gather: source size does not match the mode");
  hipStream_t s = S(stream);
  const size_t esz = dtype == 0 ? 4 : 2;
  ExScratch xs;
  void* ps = xs.get((size_t)batch * hs * ws * src_channels * esz);
  void* pd = xs.get((size_t)batch * hd * wd * cd * esz);
  MI355_REQUIRE(ps && pd, -2, "grad_gather: out of device memory");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, src, src_channels, nullptr, 0, batch, hs * ws, src_channels, ps, s))) return rc;
  if (accumulate) { if ((rc = pack_nhwc_launch(dtype, dst, cd, nullptr, 0, batch, hd * wd, cd, pd, s))) return rc; }
  else MI355_CHECK_HIP(hipMemsetAsync(pd, 0xFF, (size_t)batch * hd * wd * cd * esz, s));
  if ((rc = grad_gather_launch(dtype, pd, ps, batch, hd, wd, cd, hs, ws, src_channels, src_coff, mode, accumulate, scale, s))) return rc;
  if ((rc = unpack_nchw_launch(dtype, pd, batch, hd * wd, cd, dst, s))) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

// ---- the conv data gradient (later addition to ABI 108): conv_pack_weights_dgrad + conv_dgrad_launch, the sequence unet_backward runs per conv ----
int mi355_conv2d_vjp(const float* w_host, const float* grad_out, float* g0, float* g1, float* du_raw, int acc0, int acc1, int batch, int cout,
                     int cin, int c0, int c1, int h, int w, int ksize, int mode, int g_channels, int dtype, const mi355_debug_config* debug,
                     int32_t route[4], void* workspace, int64_t workspace_bytes, void* stream) {
  if (route) route[0] = route[1] = route[2] = route[3] = -1;
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16, -1, "conv2d_vjp: dtype must be MI355_F32 or MI355_BF16 (the backward pass has no other form)");
  const bool dry = workspace == nullptr && workspace_bytes == 0 && route != nullptr;   // route query: host code only
  MI355_REQUIRE(dry || (w_host && grad_out && workspace), -1, "conv2d_vjp: null argument");
  MI355_REQUIRE(batch > 0 && cout > 0 && cin > 0 && c0 > 0 && c1 >= 0 && h > 0 && w > 0, -1, "conv2d_vjp: bad sizes");
  MI355_REQUIRE(ksize == 1 || ksize == 3, -1, "conv2d_vjp: kernel size must be 1 or 3");
  MI355_REQUIRE(mode == CONV_UNIT || ((mode == CONV_STRIDE2 || mode == CONV_UP2) && ksize == 3), -1, "conv2d_vjp: mode 0 (unit), or with a 3x3 kernel 1 (stride 2) / 2 (nearest x2)");
  const bool raw = du_raw != nullptr;
  MI355_REQUIRE((dry || raw) ? (!g0 && !g1 && !acc0 && !acc1) : (g0 && (g1 != nullptr) == (c1 > 0)), -1, "conv2d_vjp: either du_raw alone, or g0 (and g1 with c1 > 0)");
  const int CH = dtype == 0 ? 16 : 32, V = dtype == 0 ? 4 : 8;
  const size_t esz = dtype == 0 ? 4 : 2;
  MI355_REQUIRE(c0 + c1 >= cin, -2, "conv2d_vjp: c0 + c1 must cover the conv's input channels");
  MI355_REQUIRE(c0 % V == 0 && c1 % V == 0, -2, "conv2d_vjp: c0 and c1 must be whole 16-byte channel fragments");
  MI355_REQUIRE(g_channels == (cout + CH - 1) / CH * CH, -2, "conv2d_vjp: g_channels must be cout padded to whole 64-byte chunks");
  const int cin_pad = (c0 + c1 + 31) / 32 * 32;   // the plan builder's PlanOp::cin_pad
  const int Ho = mode == CONV_STRIDE2 ? (h - 1) / 2 + 1 : (mode == CONV_UP2 ? 2 * h : h);
  const int Wo = mode == CONV_STRIDE2 ? (w - 1) / 2 + 1 : (mode == CONV_UP2 ? 2 * w : w);
  const int Hd = mode == CONV_UP2 ? Ho : h, Wd = mode == CONV_UP2 ? Wo : w;   // the data-gradient conv's own resolution
  ConvDgradDesc d; d.dtype = dtype; d.Cg = g_channels; d.Hg = Ho; d.Wg = Wo; d.cin_pad = cin_pad; d.ks = ksize; d.mode = mode;
  d.N = batch; d.Hs = h; d.Ws = w; d.knobs = debug;
  if (dry) {
    ConvRoute r;
    if (int rc = conv_dgrad_route(d, &r)) return rc;
    route[0] = r.kernel; route[1] = r.form; route[2] = r.geom.BM; route[3] = r.geom.BN;
    return 0;
  }
  hipStream_t s = S(stream);
  const size_t wbytes = conv_packed_weight_bytes_dgrad(dtype, cout, cin, ksize, cin_pad);
  char* p = reinterpret_cast<char*>(workspace);
  void* gp = p; p += al256((size_t)batch * Ho * Wo * g_channels * esz);
  void* zbuf = p; if (mode == CONV_STRIDE2) p += al256((size_t)batch * h * w * g_channels * esz);
  void* du = p; p += al256((size_t)batch * Hd * Wd * cin_pad * esz);
  void* tmp = p; if (mode == CONV_UP2 && raw) p += al256((size_t)batch * h * w * cin_pad * esz);
  void* q0 = p; if (!raw) p += al256((size_t)batch * h * w * c0 * esz);
  void* q1 = p; if (!raw && c1) p += al256((size_t)batch * h * w * c1 * esz);
  void* wdev = p; p += al256(wbytes);
  uint32_t* errw = reinterpret_cast<uint32_t*>(p); p += 256;
  MI355_REQUIRE(p <= reinterpret_cast<char*>(workspace) + workspace_bytes, -2, "conv2d_vjp: workspace too small");
  int rc;
  MI355_CHECK_HIP(hipMemsetAsync(errw, 0, 256, s));
  // the cotangent as the walker holds it: NHWC, channels cout .. g_channels zero (pack_nhwc's padding, as for the network's own cotangent)
  if ((rc = pack_nhwc_launch(dtype, grad_out, cout, nullptr, 0, batch, Ho * Wo, g_channels, gp, s))) return rc;
  // a gradient the scatter adds to is the caller's, packed; anything else stays as the caller filled the workspace
  if (acc0 && (rc = pack_nhwc_launch(dtype, g0, c0, nullptr, 0, batch, h * w, c0, q0, s))) return rc;
  if (acc1 && c1 && (rc = pack_nhwc_launch(dtype, g1, c1, nullptr, 0, batch, h * w, c1, q1, s))) return rc;
  std::vector<char> packed(wbytes);
  conv_pack_weights_dgrad(dtype, w_host, cout, cin, ksize, cin_pad, packed.data());
  MI355_CHECK_HIP(hipMemcpyAsync(wdev, packed.data(), wbytes, hipMemcpyHostToDevice, s));
  d.G = gp; d.wT = wdev; d.du = du; d.tmp = tmp; d.zbuf = zbuf; d.scatter = !raw; d.err = errw;
  if (!raw) { d.g0 = q0; d.C0 = c0; d.acc0 = acc0; if (c1) { d.g1 = q1; d.C1 = c1; d.acc1 = acc1; } }
  ConvDgradOut o;
  if ((rc = conv_dgrad_launch(d, s, &o))) return rc;
  if (route) { route[0] = o.route.kernel; route[1] = o.route.form; route[2] = o.route.geom.BM; route[3] = o.route.geom.BN; }
  if (raw) {
    if ((rc = unpack_nchw_launch(dtype, o.dU, batch, h * w, o.dU_stride, du_raw, s))) return rc;
  } else {
    if ((rc = unpack_nchw_launch(dtype, q0, batch, h * w, c0, g0, s))) return rc;
    if (c1 && (rc = unpack_nchw_launch(dtype, q1, batch, h * w, c1, g1, s))) return rc;
  }
  MI355_CHECK_HIP(hipStreamSynchronize(s));   // `packed` is a temporary host buffer
  uint32_t ev = 0;
  MI355_CHECK_HIP(hipMemcpy(&ev, errw, 4, hipMemcpyDeviceToHost));
  if (ev) { mi355_set_error("conv2d_vjp: the persistent kernel gave up a bounded counter wait (hand-over stalled): the output is invalid"); return MI355_ERR_TIMEOUT; }
  return 0;
}

// ---- one forward conv, isolated (later addition to ABI 108): mi355_conv2d_ex with the prologue's (a, b) given, the route always reported, the two
// sampler-only edge forms, and nothing initialised that no kernel writes ----
int mi355_conv2d_fwd(const float* x, const float* x1, int cin1, const float* w_host, const float* bias_host, float* y, int batch, int cin, int h,
                     int w, int cout, int ksize, int stride, int resample, const float* pro_a, const float* pro_b, int pro_silu, const float* emb,
                     const float* res, int res_mode, int flags, float* axpy_x, float axpy_scale, int dtype, const mi355_debug_config* debug,
                     int32_t route[8], void* workspace, int64_t workspace_bytes, void* stream) {
  if (route) for (int i = 0; i < 8; ++i) route[i] = -1;
  const mi355_debug_config& K = debug ? *debug : mi355_default_debug();
  const bool dry = workspace == nullptr && workspace_bytes == 0 && route != nullptr;   // route query: host code only, no pointer is read
  MI355_REQUIRE(dry || (x && w_host && y && workspace), -1, "conv2d_fwd: null argument");
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16 || dtype == MI355_BF16X2 || dtype == MI355_F16, -1, "conv2d_fwd: bad dtype");
  MI355_REQUIRE(batch > 0 && cin > 0 && cin1 >= 0 && cout > 0 && h > 0 && w > 0, -1, "conv2d_fwd: bad sizes");
  MI355_REQUIRE(ksize == 1 || ksize == 3, -1, "conv2d_fwd: kernel size must be 1 or 3");
  MI355_REQUIRE(stride == 1 || stride == 2, -1, "conv2d_fwd: stride must be 1 or 2");
  MI355_REQUIRE(resample == 0 || resample == 2, -1, "conv2d_fwd: resample must be 0 or 2 (nearest x2; pooling is a pass of its own, mi355_affine_pool)");
  MI355_REQUIRE(!(stride == 2 && resample), -1, "conv2d_fwd: stride 2 cannot be combined with resampling");
  MI355_REQUIRE((stride == 1 && !resample) || ksize == 3, -1, "conv2d_fwd: stride 2 and nearest x2 need a 3x3 kernel");
  MI355_REQUIRE((flags & ~MI355_CONV_FWD_NCHW_SRC) == 0, -1, "conv2d_fwd: unknown flag");
  MI355_REQUIRE(dry ? !x1 || cin1 > 0 : (x1 != nullptr) == (cin1 > 0), -1, "conv2d_fwd: x1 and cin1 go together");
  MI355_REQUIRE((pro_a != nullptr) == (pro_b != nullptr), -1, "conv2d_fwd: pro_a and pro_b go together");
  MI355_REQUIRE(res == nullptr || res_mode == RES_SAME || res_mode == RES_UP2, -1, "conv2d_fwd: res_mode must be 1 (same size) or 2 (nearest x2)");
  const int wsplit = dtype == MI355_BF16X2 ? 1 : 0;
  dtype = dtype == MI355_F16 ? DT_F16 : (wsplit ? DT_BF16 : dtype);   // the internal element-type code from here on (ops.h)
  const int CH = dtype == 0 ? 16 : 32, esz = dtype == 0 ? 4 : 2;
  const bool nchw_src = (flags & MI355_CONV_FWD_NCHW_SRC) != 0;   // x | x1 are the caller's NCHW tensors of the network's first conv: one packed source
  const bool two = cin1 > 0 && !nchw_src;
  MI355_REQUIRE(!two || (cin % CH == 0 && cin1 % CH == 0), -2, "conv2d_fwd: a two-source conv needs both channel counts to be multiples of the 64-byte chunk");
  MI355_REQUIRE(!nchw_src || (cin + cin1 <= 8 && !pro_a), -2, "conv2d_fwd: the NCHW source form is the first conv's: at most 8 channels in all, no prologue");
  MI355_REQUIRE(!pro_a || cin % CH == 0, -2, "conv2d_fwd: a prologue needs whole 64-byte chunks of input channels (pro_a / pro_b are [batch][cin + cin1])");
  const int c_src0 = nchw_src ? cin + cin1 : cin;
  const int cpad = (c_src0 + CH - 1) / CH * CH;
  const int ctot = cin + cin1;
  const bool nhwc = cout % 32 == 0;
  MI355_REQUIRE(nhwc || (!emb && !res), -4, "conv2d_fwd: emb / residual epilogues need an NHWC output (cout % 32 == 0)");
  MI355_REQUIRE(!axpy_x || !nhwc, -4, "conv2d_fwd: the Euler update belongs to the NCHW fp32 out conv (cout % 32 != 0)");
  static char placeholder[256];   // the route query's stand-in for every pointer the route functions test for null (never read)
  ConvDesc d; d.dtype = dtype; d.N = batch; d.Hs = h; d.Ws = w; d.C0 = cpad; d.C1 = two ? cin1 : 0; d.ks = ksize; d.Cout = cout;
  d.knobs = &K; d.wsplit = wsplit;
  if (nchw_src) d.cin_real = ctot; else if (!two && cin <= 8) d.cin_real = cin;
  d.mode = stride == 2 ? CONV_STRIDE2 : (resample == 2 ? CONV_UP2 : CONV_UNIT);
  const ConvGeom g = conv_geometry(d);
  const int Hr = res_mode == RES_UP2 ? g.Ho / 2 : g.Ho, Wr = res_mode == RES_UP2 ? g.Wo / 2 : g.Wo;
  const bool want_up2 = d.mode == CONV_UP2 && ksize == 3 && !wsplit && (K.conv_pp & 64) && cpad == c_src0;
  char* p = dry ? placeholder : reinterpret_cast<char*>(workspace);
  auto take = [&](size_t bytes) { char* q = p; if (!dry) p += al256(bytes); return (void*)q; };
  void* xin = take((size_t)batch * h * w * cpad * esz);
  void* xin1 = two ? take((size_t)batch * h * w * cin1 * esz) : nullptr;
  const size_t wbytes = conv_packed_weight_bytes(dtype, cout, ctot, ksize, wsplit);
  void* wdev = take(wbytes);
  float* bdev = reinterpret_cast<float*>(take((size_t)cout * 4));
  void* yout = nhwc ? take((size_t)batch * g.Ho * g.Wo * cout * esz) : (void*)y;
  void* rin = res ? take((size_t)batch * Hr * Wr * cout * esz) : nullptr;
  uint32_t* errw = reinterpret_cast<uint32_t*>(take(256));
  MI355_REQUIRE(dry || p <= reinterpret_cast<char*>(workspace) + workspace_bytes, -2, "conv2d_fwd: workspace too small");
  const size_t wbytes_up2 = want_up2 ? conv_packed_weight_bytes_up2(dtype, cout, ctot) : 0;
  ExScratch xs;
  void* wdev_up2 = !want_up2 ? nullptr : (dry ? (void*)placeholder : xs.get(wbytes_up2));
  MI355_REQUIRE(!want_up2 || wdev_up2, -2, "conv2d_fwd: out of device memory");
  d.src0 = xin; d.src1 = xin1; d.w = wdev; d.w_up2 = wdev_up2; d.bias = bias_host ? bdev : nullptr; d.err = errw;
  if (pro_a) { d.pro_a = pro_a; d.pro_b = pro_b; d.pro_silu = pro_silu; }
  if (emb) { d.emb = emb; d.emb_stride = cout; }
  if (res) { d.res = rin; d.res_mode = res_mode; }
  d.out_mode = nhwc ? OUT_NHWC : OUT_NCHW_F32; d.out = dry ? (void*)placeholder : yout;
  if (nchw_src) {
    d.nchw0 = dry ? reinterpret_cast<const float*>(placeholder) : x; d.nchw_c0 = cin;
    d.nchw1 = !cin1 ? nullptr : (dry ? reinterpret_cast<const float*>(placeholder) : x1); d.nchw_c1 = cin1;
  }
  if (axpy_x) { d.axpy_x = axpy_x; d.axpy_scale = axpy_scale; }
  ConvRoute r;
  int rc;
  if ((rc = conv_route(d, &r))) return rc;
  auto report = [&] {
    if (!route) return;
    route[0] = r.kernel; route[1] = r.form; route[2] = r.geom.BM; route[3] = r.geom.BN; route[4] = r.reads_nchw; route[5] = r.axpy;
    route[6] = r.ksplit; route[7] = r.n_mt;
  };
  if (dry) { report(); return 0; }
  hipStream_t s = S(stream);
  MI355_CHECK_HIP(hipMemsetAsync(errw, 0, 256, s));
  if (!r.reads_nchw) {   // a launch that reads the caller's tensors itself leaves the packed copy as the caller filled the workspace
    if ((rc = pack_nhwc_launch(dtype, x, cin, nchw_src ? x1 : nullptr, nchw_src ? cin1 : 0, batch, h * w, cpad, xin, s))) return rc;
  }
  if (two && (rc = pack_nhwc_launch(dtype, x1, cin1, nullptr, 0, batch, h * w, cin1, xin1, s))) return rc;
  if (res && (rc = pack_nhwc_launch(dtype, res, cout, nullptr, 0, batch, Hr * Wr, cout, rin, s))) return rc;
  std::vector<char> packed(wbytes), packed_up2(wbytes_up2);
  conv_pack_weights(dtype, w_host, cout, ctot, ksize, packed.data(), wsplit);
  MI355_CHECK_HIP(hipMemcpyAsync(wdev, packed.data(), wbytes, hipMemcpyHostToDevice, s));
  if (want_up2) {
    conv_pack_weights_up2(dtype, w_host, cout, ctot, packed_up2.data());
    MI355_CHECK_HIP(hipMemcpyAsync(wdev_up2, packed_up2.data(), wbytes_up2, hipMemcpyHostToDevice, s));
  }
  if (bias_host) MI355_CHECK_HIP(hipMemcpyAsync(bdev, bias_host, (size_t)cout * 4, hipMemcpyHostToDevice, s));
  if ((rc = conv_launch(d, r, s))) return rc;
  report();
  if (nhwc && (rc = unpack_nchw_launch(dtype, yout, batch, g.Ho * g.Wo, cout, y, s))) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));   // `packed` is a temporary host buffer
  uint32_t ev = 0;
  MI355_CHECK_HIP(hipMemcpy(&ev, errw, 4, hipMemcpyDeviceToHost));
  if (ev) { mi355_set_error("conv2d_fwd: the persistent kernel gave up a bounded counter wait (hand-over stalled): the output is invalid"); return MI355_ERR_TIMEOUT; }
  return 0;
}

// ---- the embedding path and the layout kernels (later additions to ABI 108): csrc/embed.hip and unpack_channels of csrc/backward.hip, each through
// its own *_launch function, nothing packed or unpacked in between; every op synchronises the stream ----
namespace {
// a pinned, mapped host word as a handle's error word is (unet_engine.hip): the kernels store into it over the bus
struct ErrWord {
  uint32_t* host = nullptr; uint32_t* dev = nullptr;
  ~ErrWord() { if (host) (void)hipHostFree(host); }
  int init() {
    MI355_CHECK_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), 64, hipHostMallocMapped));
    *host = 0u;
    MI355_CHECK_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dev), host, 0));
    return 0;
  }
};
// the ABI's dtype code -> the internal element-type code (ops.h); MI355_BF16X2 stores bf16
int layout_op_dtype(int dtype, const char* who, int* out) {
  if (dtype != MI355_F32 && dtype != MI355_BF16 && dtype != MI355_BF16X2 && dtype != MI355_F16) { mi355_set_error(std::string(who) + ": bad dtype"); return -1; }
  *out = dtype == MI355_F16 ? DT_F16 : (dtype == MI355_BF16X2 ? DT_BF16 : dtype);
  return 0;
}
}  // namespace

int mi355_linear(const float* in, const float* wt, const float* bias, float* out, int batch, int k, int j, int in_act, int out_act, int32_t* form,
                 void* stream) {
  if (form) *form = -1;
  MI355_REQUIRE(in && wt && out && batch > 0 && k > 0 && j > 0, -1, "linear: bad argument");
  hipStream_t s = S(stream);
  if (int rc = linear_launch(in, wt, bias, out, batch, k, j, in_act, out_act, s)) return rc;
  if (form) *form = linear_form(batch, k);
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int mi355_label_emb_linear(const float* h, int h_div, const float* lemb, const int32_t* labels, int n_classes, const float* wt, const float* bias,
                           float* out, int rows, int k, int j, int32_t* err_word, int32_t* form, void* stream) {
  if (form) *form = -1;
  if (err_word) *err_word = -1;
  MI355_REQUIRE(h && lemb && wt && out && err_word && k > 0 && j > 0, -1, "label_emb_linear: bad argument");
  hipStream_t s = S(stream);
  ErrWord e;
  if (int rc = e.init()) return rc;
  if (int rc = label_emb_linear_launch(h, h_div, lemb, labels, n_classes, wt, bias, out, rows, k, j, e.dev, s)) return rc;
  if (form) *form = label_emb_linear_form(k);
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  *err_word = (int32_t)*e.host;
  return 0;
}

int mi355_emb_gather(const float* table, const int32_t* labels, int n_classes, float* out, int batch, int j, int32_t* err_word, void* stream) {
  if (err_word) *err_word = -1;
  MI355_REQUIRE(err_word && j > 0, -1, "emb_gather: bad argument");
  hipStream_t s = S(stream);
  ErrWord e;
  if (int rc = e.init()) return rc;
  if (int rc = emb_gather_launch(table, labels, n_classes, out, batch, j, e.dev, s)) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  *err_word = (int32_t)*e.host;
  return 0;
}

int mi355_pack_nhwc(const float* x, int cx, const float* cond, int cc, int batch, int hw, int cpad, void* out, int dtype, void* stream) {
  MI355_REQUIRE(x && out && batch > 0 && hw > 0 && cx > 0 && cc >= 0 && (cond != nullptr) == (cc > 0), -1, "pack_nhwc: bad argument");
  MI355_REQUIRE(cpad >= cx + cc, -2, "pack_nhwc: cpad must hold cx + cc channels");
  if (int rc = layout_op_dtype(dtype, "pack_nhwc", &dtype)) return rc;
  hipStream_t s = S(stream);
  if (int rc = pack_nhwc_launch(dtype, x, cx, cond, cc, batch, hw, cpad, out, s)) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int mi355_unpack_nchw(const void* in, int batch, int hw, int channels, float* out, int dtype, void* stream) {
  MI355_REQUIRE(in && out && batch > 0 && hw > 0 && channels > 0, -1, "unpack_nchw: bad argument");
  if (int rc = layout_op_dtype(dtype, "unpack_nchw", &dtype)) return rc;
  hipStream_t s = S(stream);
  if (int rc = unpack_nchw_launch(dtype, in, batch, hw, channels, out, s)) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int mi355_unpack_channels(const void* in, int batch, int hw, int stride, int c0, int count, float* out, int dtype, void* stream) {
  MI355_REQUIRE(in && out && batch > 0 && hw > 0 && count > 0 && c0 >= 0, -1, "unpack_channels: bad argument");
  MI355_REQUIRE(c0 + count <= stride, -2, "unpack_channels: channels c0 .. c0 + count must lie inside a row");
  if (int rc = layout_op_dtype(dtype, "unpack_channels", &dtype)) return rc;
  hipStream_t s = S(stream);
  if (int rc = unpack_channels_launch(dtype, in, batch, hw, stride, c0, count, out, s)) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

int mi355_resample(const void* in, void* out, int batch, int h, int w, int channels, int mode, int dtype, void* stream) {
  MI355_REQUIRE(in && out && batch > 0 && h > 0 && w > 0 && channels > 0, -1, "resample: bad argument");
  MI355_REQUIRE(mode == CONV_UP2 || (mode == CONV_POOL2 && h >= 2 && w >= 2), -1, "resample: mode must be 2 (nearest x2) or 3 (2x2 average pool, h and w >= 2)");
  if (int rc = layout_op_dtype(dtype, "resample", &dtype)) return rc;
  hipStream_t s = S(stream);
  if (int rc = resample_launch(dtype, in, out, batch, h, w, channels, mode, s)) return rc;
  MI355_CHECK_HIP(hipStreamSynchronize(s));
  return 0;
}

}  // extern "C"
