// Single-op test harness of libmi355_sampler.so (see include/mi355_sampler.h): the kernels the network launches, one op per call, NCHW fp32 at
// the boundary (mi355_conv2d / mi355_conv2d_ex, the attention ops, the GroupNorm test ops, mi355_affine_pool, mi355_grad_gather, mi355_conv2d_vjp, mi355_conv2d_fwd).
// Every entry point validates its own arguments; what they share comes first: the dtype decode, the arena, the weight stager, the conv error word.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "capi_internal.h"

namespace {

// ---- the ABI's dtype code -> what the kernels take: the internal element-type code (ops.h; MI355_BF16X2 stores bf16, its weights as hi | lo bf16
// halves along K: wsplit), the channels of a 64-byte chunk and the element size ----
struct ElemType { int dt = DT_F32, wsplit = 0, CH = 16; size_t esz = 4; };
enum ElemSet { ELEMS_ANY, ELEMS_FWD, ELEMS_BWD };   // every code; all but MI355_BF16X2; fp32 and bf16 (what the backward kernels take)
enum { SAY_COND = 1, SAY_TERSE = 2 };               // how an op words its refusal: with the tested condition after it; in the short words of ELEMS_ANY
// 0, *e and *dtype the internal code from there on, or -1 with the refusal set: "<who>: <the set's words>", for ELEMS_BWD followed by "(<why> no other form)"
int elem_type(int* dtype, ElemSet set, const char* who, ElemType* e, int say = 0, const char* why = "") {
  static const struct { bool x2, f16; const char* words; const char* cond; } sets[3] = {
      {true, true, "bad dtype", "dtype == MI355_F32 || dtype == MI355_BF16 || dtype == MI355_BF16X2 || dtype == MI355_F16"},
      {false, true, "dtype must be MI355_F32, MI355_BF16 or MI355_F16", "dtype == MI355_F32 || dtype == MI355_BF16 || dtype == MI355_F16"},
      {false, false, "dtype must be MI355_F32 or MI355_BF16", "dtype == MI355_F32 || dtype == MI355_BF16"}};
  const auto& a = sets[set]; const int code = *dtype;
  if (code != MI355_F32 && code != MI355_BF16 && !(code == MI355_BF16X2 && a.x2) && !(code == MI355_F16 && a.f16)) {
    std::string m = std::string(who) + ": " + ((say & SAY_TERSE) ? sets[ELEMS_ANY].words : a.words);
    if (set == ELEMS_BWD) m += std::string(" (") + why + " no other form)";
    if (say & SAY_COND) m += std::string(" [") + a.cond + "]";
    mi355_set_error(m);
    return -1;
  }
  e->wsplit = code == MI355_BF16X2 ? 1 : 0;
  *dtype = e->dt = code == MI355_F16 ? DT_F16 : (e->wsplit ? DT_BF16 : code);
  e->CH = e->dt == DT_F32 ? 16 : 32; e->esz = e->dt == DT_F32 ? 4 : 2;
  return 0;
}

// ---- the memory of one op call: take() is the only way an op carves any.  Three backings: the caller's workspace (a cursor; a take past its end
// makes ok() false, and the op refuses once, in its own words), blocks of the op's own (hipMalloc, freed when the call returns; a failed one makes
// ok() false) and the route queries' placeholder (every take is the same 256 bytes, which nothing reads).  What was taken while ok() is false is
// not memory: every op tests ok() before its first launch. ----
class Arena {
 public:
  enum Backing { CALLER, OWN, DRY };
  explicit Arena(Backing b, void* workspace = nullptr, int64_t bytes = 0) : backing_(b), p_(reinterpret_cast<char*>(workspace)), left_(bytes > 0 ? (size_t)bytes : 0) {}
  Arena(const Arena&) = delete;
  ~Arena() { for (void* q : blocks_) (void)hipFree(q); }
  void* take(size_t bytes) {
    if (backing_ == DRY) return placeholder_;
    const size_t n = al256(bytes);
    char* q = p_;
    if (backing_ == OWN) {
      if (hipMalloc(reinterpret_cast<void**>(&q), bytes ? bytes : 256) != hipSuccess) { ok_ = false; return nullptr; }
      blocks_.push_back(q);
    } else if (!ok_ || n > left_) ok_ = false;
    else { p_ += n; left_ -= n; }
    return q;
  }
  template <class T> T* take(size_t bytes) { return reinterpret_cast<T*>(take(bytes)); }
  bool ok() const { return ok_; }
  // a pointer of the caller's as the route functions see it: they test it for null and, in a route query, never read it
  template <class T> T* or_placeholder(T* real) const { return backing_ == DRY ? reinterpret_cast<T*>(placeholder_) : real; }

 private:
  Backing backing_; char* p_; size_t left_; bool ok_ = true; std::vector<void*> blocks_;
  static inline char placeholder_[256];
};

// ---- host memory that asynchronous copies read: alive until the op's final synchronise ----
struct HostStage {
  std::vector<std::vector<char>> kept;
  char* buffer(size_t bytes) { kept.emplace_back(bytes); return kept.back().data(); }
  int upload(void* dev, const void* host, size_t bytes, hipStream_t s) { MI355_CHECK_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s)); return 0; }
};

// An up-sampling 3x3 conv may run in phase form (conv_pp bit 6), which reads the filter collapsed to four 2x2 phase filters: the op then stages
// that image next to the nine-tap one, and the route decides per launch which of the two is read.  c0_real: source 0's channels before padding.
bool wants_up2_image(const ConvDesc& d, int c0_real) { return d.mode == CONV_UP2 && d.ks == 3 && !d.wsplit && (d.knobs->conv_pp & 64) && d.C0 == c0_real; }

// ---- the weight images and the bias of one conv, from host memory: the constructor takes the device memory of the nine-tap image and the bias,
// take_up2() that of the collapsed nearest-x2 image (where wants_up2_image says so); stage() packs and uploads what was taken ----
struct ConvWeights : HostStage {
  int dt, cout, ctot, ks, wsplit; size_t wbytes, ubytes = 0; void* w; float* bias; void* w_up2 = nullptr;
  ConvWeights(int dt_, int cout_, int ctot_, int ks_, int wsplit_, Arena& mem)
      : dt(dt_), cout(cout_), ctot(ctot_), ks(ks_), wsplit(wsplit_), wbytes(conv_packed_weight_bytes(dt_, cout_, ctot_, ks_, wsplit_)), w(mem.take(wbytes)),
        bias(mem.take<float>((size_t)cout_ * 4)) {}
  void take_up2(Arena& mem) { ubytes = conv_packed_weight_bytes_up2(dt, cout, ctot); w_up2 = mem.take(ubytes); }
  void describe(ConvDesc& d, bool has_bias) const { d.w = w; d.w_up2 = w_up2; d.bias = has_bias ? bias : nullptr; }
  int stage(const float* w_host, const float* bias_host, hipStream_t s) {
    char* img = buffer(wbytes); char* img_up2 = buffer(ubytes);
    conv_pack_weights(dt, w_host, cout, ctot, ks, img, wsplit);
    if (int rc = upload(w, img, wbytes, s)) return rc;
    if (w_up2) conv_pack_weights_up2(dt, w_host, cout, ctot, img_up2);
    if (int rc = w_up2 ? upload(w_up2, img_up2, ubytes, s) : 0) return rc;
    return bias_host ? upload(bias, bias_host, (size_t)cout * 4, s) : 0;
  }
};

// ---- the device error word of a conv op's launches (ConvDesc::err): the persistent kernels OR 1 into it when a bounded counter wait expires ----
struct ConvErr {
  uint32_t* word = nullptr; hipStream_t s = nullptr;
  explicit ConvErr(Arena& mem) : word(mem.take<uint32_t>(256)) {}
  int zero(hipStream_t stream) { s = stream; MI355_CHECK_HIP(hipMemsetAsync(word, 0, 256, s)); return 0; }
  // the op's (or the producer's) final synchronise - what was staged from host memory may go after it - then the word
  int finish(const char* who, const char* detail = " (hand-over stalled)") {
    MI355_CHECK_HIP(hipStreamSynchronize(s));
    uint32_t ev = 0;
    MI355_CHECK_HIP(hipMemcpy(&ev, word, 4, hipMemcpyDeviceToHost));
    if (ev) { mi355_set_error(std::string(who) + ": the persistent kernel gave up a bounded counter wait" + detail + ": the output is invalid"); return MI355_ERR_TIMEOUT; }
    return 0;
  }
};

// what every op that does not hand back a running stream ends with
int synced(hipStream_t s) { MI355_CHECK_HIP(hipStreamSynchronize(s)); return 0; }

// the first n_words of (kernel, form, tile_m, tile_n, reads_nchw, axpy, ksplit, n_mt)
void report_route(const ConvRoute& r, int32_t* out, int n_words) {
  const int words[8] = {r.kernel, r.form, r.geom.BM, r.geom.BN, r.reads_nchw, r.axpy, r.ksplit, r.n_mt};
  for (int i = 0; out && i < n_words && i < 8; ++i) out[i] = words[i];
}

// the base of a forward conv's descriptor: source 0 of c0_real channels padded to whole chunks, the mode from stride / resample (2: nearest x2)
ConvDesc conv_desc(const ElemType& e, const mi355_debug_config& K, int N, int Hs, int Ws, int c0_real, int C1, int ks, int Cout, int stride, int resample) {
  ConvDesc d; d.dtype = e.dt; d.wsplit = e.wsplit; d.knobs = &K; d.N = N; d.Hs = Hs; d.Ws = Ws; d.C1 = C1; d.ks = ks; d.Cout = Cout;
  d.C0 = (c0_real + e.CH - 1) / e.CH * e.CH;
  d.mode = stride == 2 ? CONV_STRIDE2 : (resample == 2 ? CONV_UP2 : CONV_UNIT);
  if (!C1 && c0_real <= 8) d.cin_real = c0_real;   // the padding channels pack_nhwc adds are zero: conv3x3_in_kernel contracts over the first slot only
  return d;
}

// diagnostic (mi355_debug_config::conv_time_reps): average duration of the conv launch alone
int time_conv_launch(const ConvDesc& d, const ConvRoute& route, const ConvGeom& g, int ctot, hipStream_t s) {
  const int reps = d.knobs->conv_time_reps; int rc;
  hipEvent_t e0, e1;
  MI355_CHECK_HIP(hipEventCreate(&e0)); MI355_CHECK_HIP(hipEventCreate(&e1));
  MI355_CHECK_HIP(hipEventRecord(e0, s));
  ConvRoute plain = route; plain.act_done = 0;   // the same kernel without the fused GroupNorm sites
  for (int i = 0; i < reps; ++i) if ((rc = conv_launch(d, plain, s))) return rc;
  MI355_CHECK_HIP(hipEventRecord(e1, s));
  MI355_CHECK_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  MI355_CHECK_HIP(hipEventElapsedTime(&ms, e0, e1));
  const double us = 1e3 * ms / reps, fl = 2.0 * d.N * g.Ho * g.Wo * (double)d.Cout * ctot * d.ks * d.ks;
  fprintf(stderr, "[conv time] %d launches, %.1f us each, %.0f TFLOP/s\n", reps, us, fl / us * 1e-6);
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  return 0;
}

#ifdef CONV_STAMPS
// diagnostic builds: the in-kernel clock ([4096 waves][shader cycles, 100-MHz ticks]: CLK_FLUSH) and the per-wave phase stamps of mi355_conv2d's launch
struct ConvStamps {
  size_t nwaves = 0; unsigned long long* clk = nullptr; void* waves = nullptr;
  int carve(Arena& ws, const ConvGeom& g, ConvDesc& d, hipStream_t s) {
    nwaves = (size_t)g.grid_m * g.grid_n * 4;
    clk = ws.take<unsigned long long>(65536);
    waves = ws.take(nwaves * 64);   // whole 256-byte units: right behind the clock
    MI355_REQUIRE(ws.ok(), -2, "conv2d: workspace too small (stamps)");
    MI355_CHECK_HIP(hipMemsetAsync(clk, 0, 65536 + nwaves * 64, s));
    d.dbg = waves;
    return 0;
  }
  int report(const ConvGeom& g, const mi355_debug_config& K) const {
    std::vector<unsigned long long> hv(nwaves * 8);
    MI355_CHECK_HIP(hipMemcpy(hv.data(), waves, nwaves * 64, hipMemcpyDeviceToHost));
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
    return 0;
  }
};
#endif

}  // namespace

extern "C" {

int64_t mi355_op_workspace_bytes(int batch, int max_channels, int hw) {
  const size_t c = (size_t)max_channels + 32;
  return (int64_t)(2 * al256((size_t)batch * hw * 4 * c * 4) + al256(c * c * 9 * 4 * 2) + 4 * al256((size_t)batch * c * 4) + (1 << 20));
}

static int conv2d_impl(const float* x, const float* x1, int cin1, const float* w_host, const float* bias_host, float* y, int batch, int cin,
                       int h, int w, int cout, int ksize, int stride, int resample, const float* gn_gamma, const float* gn_beta, int gn_silu,
                       const float* emb, const float* res, int res_mode, int dtype, const mi355_debug_config* debug, void* workspace,
                       int64_t workspace_bytes, void* stream, mi355_conv_extras* ex) {
  const mi355_debug_config& K = debug ? *debug : mi355_default_debug();
  MI355_REQUIRE(x && w_host && y && workspace, -1, "conv2d: null argument");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_ANY, "conv2d", &e, SAY_COND)) return rc;
  const int wsplit = e.wsplit, CH = e.CH; const size_t esz = e.esz;
  MI355_REQUIRE(stride == 1 || stride == 2, -1, "conv2d: stride must be 1 or 2");
  MI355_REQUIRE(!(stride == 2 && resample), -1, "conv2d: stride 2 cannot be combined with resampling");
  MI355_REQUIRE((x1 != nullptr) == (cin1 > 0), -1, "conv2d: x1 and cin1 go together");
  MI355_REQUIRE(res == nullptr || res_mode == RES_SAME || res_mode == RES_UP2, -1, "conv2d: res_mode must be 1 (same size) or 2 (nearest x2)");
  hipStream_t s = S(stream);
  MI355_REQUIRE(!x1 || (cin % CH == 0 && cin1 % CH == 0), -2, "conv2d: a two-source conv needs both channel counts to be multiples of the 64-byte chunk");
  const bool pool = resample == 3;   // 2x2 average pool of the (normalised) input: a pre-pass, then a plain conv
  MI355_REQUIRE(!(pool && x1), -4, "conv2d: pooling over a channel concat is not supported");
  ConvDesc d = conv_desc(e, K, batch, pool ? h / 2 : h, pool ? w / 2 : w, cin, cin1, ksize, cout, stride, resample);
  const int cpad = d.C0, ctot = cin + cin1, ctot_pad = cpad + cin1;
  const ConvGeom g = conv_geometry(d);
  const bool nhwc = cout % 32 == 0;
  MI355_REQUIRE(nhwc || (!emb && !res), -4, "conv2d: emb / residual epilogues need an NHWC output (cout % 32 == 0)");
  const int Hr = res_mode == RES_UP2 ? g.Ho / 2 : g.Ho, Wr = res_mode == RES_UP2 ? g.Wo / 2 : g.Wo;
  // ---- carve: the caller's workspace; the collapsed weight image and the extras' scratch are the op's own ----
  Arena ws(Arena::CALLER, workspace, workspace_bytes), own(Arena::OWN);
  void* xin = ws.take((size_t)batch * h * w * cpad * esz);
  void* xin1 = x1 ? ws.take((size_t)batch * h * w * cin1 * esz) : nullptr;
  ConvWeights wt(dtype, cout, ctot, ksize, wsplit, ws);
  float* ga = ws.take<float>((size_t)batch * ctot_pad * 4);
  float* gb = ws.take<float>((size_t)batch * ctot_pad * 4);
  void* yout = ws.take((size_t)batch * g.Ho * g.Wo * cout * esz);
  void* rin = res ? ws.take((size_t)batch * Hr * Wr * cout * esz) : nullptr;
  void* xpool = pool ? ws.take((size_t)batch * (h / 2) * (w / 2) * cpad * esz) : nullptr;
  ConvErr err(ws);
  MI355_REQUIRE(ws.ok(), -2, "conv2d: workspace too small");
  if (wants_up2_image(d, cin)) wt.take_up2(own);
  MI355_REQUIRE(own.ok(), -2, "conv2d: out of device memory");
  wt.describe(d, bias_host != nullptr);
  int rc;
  if ((rc = err.zero(s))) return rc;
  d.err = err.word;
  if ((rc = pack_nhwc_launch(dtype, x, cin, nullptr, 0, batch, h * w, cpad, xin, s))) return rc;
  if (x1 && (rc = pack_nhwc_launch(dtype, x1, cin1, nullptr, 0, batch, h * w, cin1, xin1, s))) return rc;
  if (res && (rc = pack_nhwc_launch(dtype, res, cout, nullptr, 0, batch, Hr * Wr, cout, rin, s))) return rc;
  if ((rc = wt.stage(w_host, bias_host, s))) return rc;
  // ---- optional parts: the derived GroupNorm32 prologue, the pooling pre-pass, the epilogue's terms ----
  if (gn_gamma) {
    MI355_REQUIRE(ctot % 32 == 0 && cin % 32 == 0, -2, "conv2d: the GroupNorm32 prologue needs channels % 32 == 0");
    GnDesc gd; gd.dtype = dtype; gd.src0 = xin; gd.C0 = cpad; gd.src1 = x1 ? xin1 : nullptr; gd.C1 = cin1; gd.N = batch; gd.HW = h * w;
    gd.gamma = gn_gamma; gd.beta = gn_beta; gd.a = ga; gd.b = gb;
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
  }
  d.out_mode = nhwc ? OUT_NHWC : OUT_NCHW_F32; d.out = nhwc ? yout : (void*)y;
#ifdef CONV_STAMPS
  ConvStamps stamps;
  if ((rc = stamps.carve(ws, g, d, s))) return rc;
#endif
  // ---- extras (mi355_conv2d_ex): the small-level kernel's fused forms, as the engine's walker asks for them ----
  bool ex_stats = false; void* act_dev[2] = {nullptr, nullptr};
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
      void* k0 = own.take((size_t)batch * h * w * ex->skip_c0 * esz);
      void* k1 = ex->skip_x1 ? own.take((size_t)batch * h * w * ex->skip_c1 * esz) : nullptr;
      const size_t fb = conv_packed_weight_bytes_skip(dtype, cout, ctot, cs);
      void* wf = own.take(fb);
      MI355_REQUIRE(own.ok(), -2, "conv2d_ex: out of device memory");
      if ((rc = pack_nhwc_launch(dtype, ex->skip_x0, ex->skip_c0, nullptr, 0, batch, h * w, ex->skip_c0, k0, s))) return rc;
      if (k1 && (rc = pack_nhwc_launch(dtype, ex->skip_x1, ex->skip_c1, nullptr, 0, batch, h * w, ex->skip_c1, k1, s))) return rc;
      char* img = wt.buffer(fb);   // both filters in one image, the summed bias over the conv's own
      conv_pack_weights_skip(dtype, w_host, ex->skip_w_host, cout, ctot, cs, img);
      if ((rc = wt.upload(wf, img, fb, s))) return rc;
      float* bias_f = reinterpret_cast<float*>(wt.buffer((size_t)cout * 4));
      for (int i = 0; i < cout; ++i) bias_f[i] = (bias_host ? bias_host[i] : 0.f) + (ex->skip_bias_host ? ex->skip_bias_host[i] : 0.f);
      if ((rc = wt.upload(wt.bias, bias_f, (size_t)cout * 4, s))) return rc;
      d.w = wf; d.bias = wt.bias;
      d.skip_src0 = k0; d.skip_C0 = ex->skip_c0; d.skip_src1 = k1; d.skip_C1 = ex->skip_c1;
    }
    for (int k = 0; k < 2; ++k) {
      if (!ex->act_out[k]) continue;
      MI355_REQUIRE(k == 0 || ex->act_out[0], -1, "conv2d_ex: site 1 without site 0");
      MI355_REQUIRE(ex->act_gamma[k] && ex->act_beta[k] && ex->act_ctotal[k] % 32 == 0 && ex->act_coff[k] >= 0 && ex->act_coff[k] + cout <= ex->act_ctotal[k], -1, "conv2d_ex: bad GroupNorm site");
      const size_t ab = (size_t)batch * g.Ho * g.Wo * ex->act_ctotal[k] * esz;
      act_dev[k] = own.take(ab);
      MI355_REQUIRE(own.ok(), -2, "conv2d_ex: out of device memory");
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
    const int cap = gn_stats_cap(g.Ho * g.Wo);
    const size_t sb = (size_t)batch * cap * (cout / 4) * 2 * 4;
    float* st = own.take<float>(sb);
    MI355_REQUIRE(own.ok(), -2, "conv2d_ex: out of device memory");
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
    report_route(route, ex->route, 4);
    for (int k = 0; k < 2; ++k)
      if (act_dev[k] && (route.act_done & (1 << k)) && (rc = unpack_nchw_launch(dtype, act_dev[k], batch, g.Ho * g.Wo, ex->act_ctotal[k], ex->act_out[k], s))) return rc;
  }
  if (K.conv_time_reps > 0 && (rc = time_conv_launch(d, route, g, ctot, s))) return rc;
  if (nhwc && (rc = unpack_nchw_launch(dtype, yout, batch, g.Ho * g.Wo, cout, y, s))) return rc;
  if ((rc = err.finish("conv2d"))) return rc;
#ifdef CONV_STAMPS
  if ((rc = stamps.report(g, K))) return rc;
#endif
  return 0;
}

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

int mi355_qkv_attention(const float* qkv, float* out, int batch, int heads, int head_channels, int length, int new_order, int dtype,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(qkv && out && workspace, -1, "qkv_attention: null argument");
  hipStream_t s = S(stream);
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_FWD, "qkv_attention", &e, SAY_COND | SAY_TERSE)) return rc;
  const size_t esz = e.esz; const int C = heads * head_channels;
  Arena ws(Arena::CALLER, workspace, workspace_bytes);
  void* qin = ws.take((size_t)batch * length * 3 * C * esz);
  void* o = ws.take((size_t)batch * length * C * esz);
  MI355_REQUIRE(ws.ok(), -2, "qkv_attention: workspace too small");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, qkv, 3 * C, nullptr, 0, batch, length, 3 * C, qin, s))) return rc;
  AttnDesc a; a.dtype = dtype; a.qkv = qin; a.out = o; a.N = batch; a.T = length; a.heads = heads; a.ch = head_channels; a.new_order = new_order;
  if ((rc = attention_launch(a, s))) return rc;
  return unpack_nchw_launch(dtype, o, batch, length, C, out, s);
}

int mi355_qkv_attention_vjp(const float* qkv, const float* grad_out, float* grad_qkv, int batch, int heads, int head_channels, int length,
                            int new_order, int dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(qkv && grad_out && grad_qkv && workspace, -1, "qkv_attention_vjp: null argument");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_BWD, "qkv_attention_vjp", &e, SAY_COND, "the attention backward has")) return rc;
  MI355_REQUIRE(batch > 0 && heads > 0 && head_channels > 0 && length > 0, -1, "qkv_attention_vjp: bad sizes");
  hipStream_t s = S(stream);
  const size_t esz = e.esz; const int C = heads * head_channels;
  const size_t rows = (size_t)batch * length;
  Arena ws(Arena::CALLER, workspace, workspace_bytes);
  void* qin = ws.take(rows * 3 * C * esz);
  void* din = ws.take(rows * C * esz);
  void* a = ws.take(rows * C * esz);
  void* dq = ws.take(rows * 3 * C * esz);
  float* Ls = ws.take<float>((size_t)batch * heads * length * 4);
  float* Ds = ws.take<float>((size_t)batch * heads * length * 4);
  MI355_REQUIRE(ws.ok(), -2, "qkv_attention_vjp: workspace too small");
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
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_FWD, "attn_block_fused", &e, SAY_COND)) return rc;
  MI355_REQUIRE(batch > 0 && channels > 0 && length > 0 && heads > 0, -1, "attn_block_fused: bad sizes");
  hipStream_t s = S(stream);
  const int C = channels;
  AttnFusedDesc d; d.dtype = dtype; d.N = batch; d.T = length; d.C = C; d.heads = heads; d.ch = C / heads; d.new_order = new_order;
  d.knobs = debug; d.form = form;
  // a shape the fused kernels do not take is the launcher's own refusal, before anything is enqueued
  if (!attn_fused_eligible(d.dtype, d.T, d.C, d.heads, d.ch, d.knobs)) return attn_fused_launch(d, s);
  const size_t esz = e.esz;
  Arena ws(Arena::CALLER, workspace, workspace_bytes);
  void* xin = ws.take((size_t)batch * length * C * esz);
  void* o = ws.take((size_t)batch * length * C * esz);
  ConvWeights wt(dtype, 3 * C, C, 1, 0, ws);   // the qkv projection: a 1x1 conv's image
  MI355_REQUIRE(ws.ok(), -2, "attn_block_fused: workspace too small");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, x, C, nullptr, 0, batch, length, C, xin, s))) return rc;
  if ((rc = wt.stage(w_host, bias_host, s))) return rc;
  MI355_CHECK_HIP(hipMemsetAsync(o, 0xFF, (size_t)batch * length * C * esz, s));   // NaN in every element type until the kernel writes it
  d.x = xin; d.ga = a; d.gb = b; d.w = wt.w; d.bias = wt.bias; d.out = o;
  if ((rc = attn_fused_launch(d, s))) return rc;
  if ((rc = unpack_nchw_launch(dtype, o, batch, length, C, out, s))) return rc;
  return synced(s);   // the weight image is staged from host memory
}

// ---- GroupNorm test ops (ABI 107): the kernels the network launches, one op each, NCHW fp32 at the boundary ------------------------
// Device scratch is the op's own (Arena::OWN); every op synchronises the stream before it returns.
int mi355_gn_affine(const float* x, const float* x1, const float* gamma, const float* beta, const float* film, float eps, float* a, float* b,
                    float* mean, float* rstd, float* y, int y_silu, int32_t* form, int batch, int c0, int c1, int hw, int dtype, void* stream) {
  MI355_REQUIRE(x && gamma && beta && a && b && batch > 0 && c0 > 0 && c1 >= 0 && hw > 0, -1, "gn_affine: bad argument");
  MI355_REQUIRE((x1 != nullptr) == (c1 > 0) && (mean != nullptr) == (rstd != nullptr), -1, "gn_affine: x1 / c1 and mean / rstd go together");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_FWD, "gn_affine", &e)) return rc;
  hipStream_t s = S(stream);
  const size_t esz = e.esz;
  const int C = c0 + c1;
  Arena xs(Arena::OWN);
  void* p0 = xs.take((size_t)batch * hw * c0 * esz);
  void* p1 = x1 ? xs.take((size_t)batch * hw * c1 * esz) : nullptr;
  void* py = y ? xs.take((size_t)batch * hw * C * esz) : nullptr;
  MI355_REQUIRE(xs.ok(), -2, "gn_affine: out of device memory");
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
  return synced(s);
}

int mi355_conv2d_gn(const float* x0, const float* w0_host, const float* bias0_host, float* y0, int cin0, int cout0, const float* x1,
                    const float* w1_host, const float* bias1_host, float* y1, int cin1, int cout1, int batch, int h, int w, int ksize, int stride,
                    int resample, const float* gamma, const float* beta, const float* film, float eps, float* a, float* b, int dtype,
                    const mi355_debug_config* debug, int32_t info[6], void* stream) {
  const mi355_debug_config& K = debug ? *debug : mi355_default_debug();
  MI355_REQUIRE(x0 && w0_host && y0 && gamma && beta && a && b && info && batch > 0, -1, "conv2d_gn: bad argument");
  MI355_REQUIRE((x1 != nullptr) == (cout1 > 0) && (!x1 || (w1_host && y1 && cin1 > 0)), -1, "conv2d_gn: the second producer needs x1, w1, y1, cin1 and cout1");
  MI355_REQUIRE((stride == 1 || stride == 2) && (resample == 0 || resample == 2) && !(stride == 2 && resample), -1, "conv2d_gn: stride 1 or 2, resample 0 or 2 (nearest x2)");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_FWD, "conv2d_gn", &e)) return rc;
  hipStream_t s = S(stream);
  const size_t esz = e.esz;
  Arena xs(Arena::OWN);
  const float* xin[2] = {x0, x1}; const float* wh[2] = {w0_host, w1_host}; const float* bh[2] = {bias0_host, bias1_host};
  float* yo[2] = {y0, y1}; const int cin[2] = {cin0, cin1}, cout[2] = {cout0, cout1};
  void* out_dev[2] = {nullptr, nullptr}; float* st[2] = {nullptr, nullptr};
  int Ho = 0, Wo = 0, rc;
  for (int i = 0; i < 6; ++i) info[i] = 0;
  for (int k = 0; k < (x1 ? 2 : 1); ++k) {   // the producers, one after the other: each a whole conv op with the statistics of its output
    MI355_REQUIRE(cout[k] % 32 == 0, -2, "conv2d_gn: NHWC outputs need cout % 32 == 0");
    ConvDesc d = conv_desc(e, K, batch, h, w, cin[k], 0, ksize, cout[k], stride, resample);
    const int cpad = d.C0; const ConvGeom g = conv_geometry(d);
    MI355_REQUIRE(k == 0 || (g.Ho == Ho && g.Wo == Wo), -2, "conv2d_gn: the producers' outputs differ in size");
    Ho = g.Ho; Wo = g.Wo;
    void* xd = xs.take((size_t)batch * h * w * cpad * esz);
    ConvWeights wt(dtype, cout[k], cin[k], ksize, 0, xs);
    if (wants_up2_image(d, cin[k])) wt.take_up2(xs);
    wt.describe(d, bh[k] != nullptr);
    out_dev[k] = xs.take((size_t)batch * Ho * Wo * cout[k] * esz);
    const int cap = gn_stats_cap(Ho * Wo);
    const size_t sb = (size_t)batch * cap * (cout[k] / 4) * 2 * 4;
    st[k] = xs.take<float>(sb);
    ConvErr err(xs);
    MI355_REQUIRE(xs.ok(), -2, "conv2d_gn: out of device memory");
    if ((rc = err.zero(s))) return rc;
    MI355_CHECK_HIP(hipMemsetAsync(st[k], 0xFF, sb, s));   // a slot no wave writes stays NaN
    if ((rc = pack_nhwc_launch(dtype, xin[k], cin[k], nullptr, 0, batch, h * w, cpad, xd, s))) return rc;
    if ((rc = wt.stage(wh[k], bh[k], s))) return rc;
    d.src0 = xd; d.out = out_dev[k]; d.out_mode = OUT_NHWC; d.err = err.word;
    d.gn_stats = st[k]; d.gn_slots_cap = cap;
    ConvRoute route;
    if ((rc = conv_route(d, &route)) || (rc = conv_launch(d, route, s))) return rc;
    info[3 * k] = route.kernel; info[3 * k + 1] = route.gn_slots; info[3 * k + 2] = route.form;
    if ((rc = unpack_nchw_launch(dtype, out_dev[k], batch, Ho * Wo, cout[k], yo[k], s))) return rc;
    if ((rc = err.finish("conv2d_gn", ""))) return rc;
  }
  if (info[1] > 0 && (!x1 || info[4] > 0)) {
    GnFinDesc f; f.stats0 = st[0]; f.slots0 = info[1]; f.C0 = cout0;
    if (x1) { f.stats1 = st[1]; f.slots1 = info[4]; f.C1 = cout1; }
    f.N = batch; f.HW = Ho * Wo; f.eps = eps; f.gamma = gamma; f.beta = beta; f.film = film; f.film_stride = film ? 2 * (cout0 + cout1) : 0;
    f.a = a; f.b = b; f.dtype = dtype; f.src0 = out_dev[0]; f.src1 = out_dev[1];
    if ((rc = gn_finalize_launch(f, s))) return rc;
  }
  return synced(s);
}

int mi355_affine_pool(const float* x, const float* a, const float* b, int silu, float* out, int batch, int channels, int h, int w, int dtype,
                      void* stream) {
  MI355_REQUIRE(x && out && (a != nullptr) == (b != nullptr) && batch > 0 && channels > 0 && h > 0 && w > 0, -1, "affine_pool: bad argument");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_FWD, "affine_pool", &e)) return rc;
  hipStream_t s = S(stream);
  const size_t esz = e.esz;
  Arena xs(Arena::OWN);
  void* pi = xs.take((size_t)batch * h * w * channels * esz);
  void* po = xs.take((size_t)batch * (h / 2) * (w / 2) * channels * esz);
  MI355_REQUIRE(xs.ok(), -2, "affine_pool: out of device memory");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, x, channels, nullptr, 0, batch, h * w, channels, pi, s))) return rc;
  MI355_CHECK_HIP(hipMemsetAsync(po, 0xFF, (size_t)batch * (h / 2) * (w / 2) * channels * esz, s));
  if ((rc = affine_pool_launch(dtype, pi, a, b, silu, po, batch, h, w, channels, s))) return rc;
  if ((rc = unpack_nchw_launch(dtype, po, batch, (h / 2) * (w / 2), channels, out, s))) return rc;
  return synced(s);
}

int mi355_gn_silu_vjp(const float* x0, const float* x1, const float* gamma, const float* beta, const float* film, float eps, int silu,
                      const float* du, int du_stride, float* g0, float* g1, int acc0, int acc1, int batch, int c0, int c1, int hw, int dtype,
                      void* stream) {
  MI355_REQUIRE(x0 && gamma && beta && du && g0 && batch > 0 && c0 > 0 && c1 >= 0 && hw > 0, -1, "gn_silu_vjp: bad argument");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_BWD, "gn_silu_vjp", &e, SAY_COND, "the GroupNorm backward has")) return rc;
  MI355_REQUIRE((x1 != nullptr) == (c1 > 0) && (x1 != nullptr) == (g1 != nullptr), -1, "gn_silu_vjp: x1, g1 and c1 go together");
  const int C = c0 + c1;
  MI355_REQUIRE(du_stride >= C, -2, "gn_silu_vjp: du_stride must be at least c0 + c1");
  hipStream_t s = S(stream);
  const size_t esz = e.esz;
  Arena xs(Arena::OWN);
  void* p0 = xs.take((size_t)batch * hw * c0 * esz);
  void* p1 = x1 ? xs.take((size_t)batch * hw * c1 * esz) : nullptr;
  void* pd = xs.take((size_t)batch * hw * du_stride * esz);
  void* q0 = xs.take((size_t)batch * hw * c0 * esz);
  void* q1 = x1 ? xs.take((size_t)batch * hw * c1 * esz) : nullptr;
  float* ab = xs.take<float>(((size_t)2 * batch * C + (size_t)2 * batch * 32) * 4);
  MI355_REQUIRE(xs.ok(), -2, "gn_silu_vjp: out of device memory");
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
  return synced(s);
}

int mi355_grad_gather(const float* src, float* dst, int batch, int cd, int hd, int wd, int hs, int ws, int src_channels, int src_coff, int mode,
                      int accumulate, float scale, int dtype, void* stream) {
  MI355_REQUIRE(src && dst && batch > 0 && cd > 0 && hd > 0 && wd > 0 && hs > 0 && ws > 0, -1, "grad_gather: bad argument");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_BWD, "grad_gather", &e, SAY_COND, "the gather kernels have")) return rc;
  MI355_REQUIRE(src_coff >= 0 && src_coff + cd <= src_channels, -2, "grad_gather: channels src_coff .. src_coff + cd must lie inside the source");
  // every source pixel the mode reads must exist (the kernel does not clamp): identity; 2x2 blocks; half-resolution; zero insertion (any source size)
  const bool fits = mode == GATHER_SAME ? (hs == hd && ws == wd) : mode == GATHER_POOL ? (hs == 2 * hd && ws == 2 * wd)
                  : mode == GATHER_UP ? (2 * hs >= hd && 2 * ws >= wd) : mode == GATHER_STUFF;
  MI355_REQUIRE(fits, -2, "grad_gather: source size does not match the mode");
  hipStream_t s = S(stream);
  const size_t esz = e.esz;
  Arena xs(Arena::OWN);
  void* ps = xs.take((size_t)batch * hs * ws * src_channels * esz);
  void* pd = xs.take((size_t)batch * hd * wd * cd * esz);
  MI355_REQUIRE(xs.ok(), -2, "grad_gather: out of device memory");
  int rc;
  if ((rc = pack_nhwc_launch(dtype, src, src_channels, nullptr, 0, batch, hs * ws, src_channels, ps, s))) return rc;
  if (accumulate) { if ((rc = pack_nhwc_launch(dtype, dst, cd, nullptr, 0, batch, hd * wd, cd, pd, s))) return rc; }
  else MI355_CHECK_HIP(hipMemsetAsync(pd, 0xFF, (size_t)batch * hd * wd * cd * esz, s));
  if ((rc = grad_gather_launch(dtype, pd, ps, batch, hd, wd, cd, hs, ws, src_channels, src_coff, mode, accumulate, scale, s))) return rc;
  if ((rc = unpack_nchw_launch(dtype, pd, batch, hd * wd, cd, dst, s))) return rc;
  return synced(s);
}

// ---- the conv data gradient (later addition to ABI 108): conv_pack_weights_dgrad + conv_dgrad_launch, the sequence unet_backward runs per conv ----
int mi355_conv2d_vjp(const float* w_host, const float* grad_out, float* g0, float* g1, float* du_raw, int acc0, int acc1, int batch, int cout,
                     int cin, int c0, int c1, int h, int w, int ksize, int mode, int g_channels, int dtype, const mi355_debug_config* debug,
                     int32_t route[4], void* workspace, int64_t workspace_bytes, void* stream) {
  if (route) route[0] = route[1] = route[2] = route[3] = -1;
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_BWD, "conv2d_vjp", &e, SAY_COND, "the backward pass has")) return rc;
  const bool dry = workspace == nullptr && workspace_bytes == 0 && route != nullptr;   // route query: host code only
  MI355_REQUIRE(dry || (w_host && grad_out && workspace), -1, "conv2d_vjp: null argument");
  MI355_REQUIRE(batch > 0 && cout > 0 && cin > 0 && c0 > 0 && c1 >= 0 && h > 0 && w > 0, -1, "conv2d_vjp: bad sizes");
  MI355_REQUIRE(ksize == 1 || ksize == 3, -1, "conv2d_vjp: kernel size must be 1 or 3");
  MI355_REQUIRE(mode == CONV_UNIT || ((mode == CONV_STRIDE2 || mode == CONV_UP2) && ksize == 3), -1, "conv2d_vjp: mode 0 (unit), or with a 3x3 kernel 1 (stride 2) / 2 (nearest x2)");
  const bool raw = du_raw != nullptr;
  MI355_REQUIRE((dry || raw) ? (!g0 && !g1 && !acc0 && !acc1) : (g0 && (g1 != nullptr) == (c1 > 0)), -1, "conv2d_vjp: either du_raw alone, or g0 (and g1 with c1 > 0)");
  const int CH = e.CH, V = dtype == 0 ? 4 : 8; const size_t esz = e.esz;
  MI355_REQUIRE(c0 + c1 >= cin, -2, "conv2d_vjp: c0 + c1 must cover the conv's input channels");
  MI355_REQUIRE(c0 % V == 0 && c1 % V == 0, -2, "conv2d_vjp: c0 and c1 must be whole 16-byte channel fragments");
  MI355_REQUIRE(g_channels == (cout + CH - 1) / CH * CH, -2, "conv2d_vjp: g_channels must be cout padded to whole 64-byte chunks");
  const int cin_pad = conv_dgrad_cin_pad(c0, c1);
  const int Ho = mode == CONV_STRIDE2 ? (h - 1) / 2 + 1 : (mode == CONV_UP2 ? 2 * h : h);
  const int Wo = mode == CONV_STRIDE2 ? (w - 1) / 2 + 1 : (mode == CONV_UP2 ? 2 * w : w);
  const int Hd = mode == CONV_UP2 ? Ho : h, Wd = mode == CONV_UP2 ? Wo : w;   // the data-gradient conv's own resolution
  ConvDgradDesc d; d.dtype = dtype; d.Cg = g_channels; d.Hg = Ho; d.Wg = Wo; d.cin_pad = cin_pad; d.ks = ksize; d.mode = mode;
  d.N = batch; d.Hs = h; d.Ws = w; d.knobs = debug;
  if (dry) {
    ConvRoute r;
    if (int rc = conv_dgrad_route(d, &r)) return rc;
    report_route(r, route, 4);
    return 0;
  }
  hipStream_t s = S(stream);
  const size_t wbytes = conv_packed_weight_bytes_dgrad(dtype, cout, cin, ksize, cin_pad);
  Arena ws(Arena::CALLER, workspace, workspace_bytes);
  void* gp = ws.take((size_t)batch * Ho * Wo * g_channels * esz);
  void* zbuf = mode == CONV_STRIDE2 ? ws.take((size_t)batch * h * w * g_channels * esz) : nullptr;
  void* du = ws.take((size_t)batch * Hd * Wd * cin_pad * esz);
  void* tmp = mode == CONV_UP2 && raw ? ws.take((size_t)batch * h * w * cin_pad * esz) : nullptr;
  void* q0 = !raw ? ws.take((size_t)batch * h * w * c0 * esz) : nullptr;
  void* q1 = !raw && c1 ? ws.take((size_t)batch * h * w * c1 * esz) : nullptr;
  void* wdev = ws.take(wbytes);
  ConvErr err(ws);
  MI355_REQUIRE(ws.ok(), -2, "conv2d_vjp: workspace too small");
  int rc;
  if ((rc = err.zero(s))) return rc;
  // the cotangent as the walker holds it: NHWC, channels cout .. g_channels zero (pack_nhwc's padding, as for the network's own cotangent)
  if ((rc = pack_nhwc_launch(dtype, grad_out, cout, nullptr, 0, batch, Ho * Wo, g_channels, gp, s))) return rc;
  // a gradient the scatter adds to is the caller's, packed; anything else stays as the caller filled the workspace
  if (acc0 && (rc = pack_nhwc_launch(dtype, g0, c0, nullptr, 0, batch, h * w, c0, q0, s))) return rc;
  if (acc1 && c1 && (rc = pack_nhwc_launch(dtype, g1, c1, nullptr, 0, batch, h * w, c1, q1, s))) return rc;
  HostStage host;
  char* img = host.buffer(wbytes);
  conv_pack_weights_dgrad(dtype, w_host, cout, cin, ksize, cin_pad, img);
  if ((rc = host.upload(wdev, img, wbytes, s))) return rc;
  d.G = gp; d.wT = wdev; d.du = du; d.tmp = tmp; d.zbuf = zbuf; d.scatter = !raw; d.err = err.word;
  if (!raw) { d.g0 = q0; d.C0 = c0; d.acc0 = acc0; if (c1) { d.g1 = q1; d.C1 = c1; d.acc1 = acc1; } }
  ConvDgradOut o;
  if ((rc = conv_dgrad_launch(d, s, &o))) return rc;
  report_route(o.route, route, 4);
  if (raw) {
    if ((rc = unpack_nchw_launch(dtype, o.dU, batch, h * w, o.dU_stride, du_raw, s))) return rc;
  } else {
    if ((rc = unpack_nchw_launch(dtype, q0, batch, h * w, c0, g0, s))) return rc;
    if (c1 && (rc = unpack_nchw_launch(dtype, q1, batch, h * w, c1, g1, s))) return rc;
  }
  return err.finish("conv2d_vjp");
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
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_ANY, "conv2d_fwd", &e, SAY_COND)) return rc;
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
  const int CH = e.CH; const size_t esz = e.esz;
  const bool nchw_src = (flags & MI355_CONV_FWD_NCHW_SRC) != 0;   // x | x1 are the caller's NCHW tensors of the network's first conv: one packed source
  const bool two = cin1 > 0 && !nchw_src;
  MI355_REQUIRE(!two || (cin % CH == 0 && cin1 % CH == 0), -2, "conv2d_fwd: a two-source conv needs both channel counts to be multiples of the 64-byte chunk");
  MI355_REQUIRE(!nchw_src || (cin + cin1 <= 8 && !pro_a), -2, "conv2d_fwd: the NCHW source form is the first conv's: at most 8 channels in all, no prologue");
  MI355_REQUIRE(!pro_a || cin % CH == 0, -2, "conv2d_fwd: a prologue needs whole 64-byte chunks of input channels (pro_a / pro_b are [batch][cin + cin1])");
  const int c_src0 = nchw_src ? cin + cin1 : cin;
  const int ctot = cin + cin1;
  const bool nhwc = cout % 32 == 0;
  MI355_REQUIRE(nhwc || (!emb && !res), -4, "conv2d_fwd: emb / residual epilogues need an NHWC output (cout % 32 == 0)");
  MI355_REQUIRE(!axpy_x || !nhwc, -4, "conv2d_fwd: the Euler update belongs to the NCHW fp32 out conv (cout % 32 != 0)");
  ConvDesc d = conv_desc(e, K, batch, h, w, c_src0, two ? cin1 : 0, ksize, cout, stride, resample);
  const int cpad = d.C0; const ConvGeom g = conv_geometry(d);
  const int Hr = res_mode == RES_UP2 ? g.Ho / 2 : g.Ho, Wr = res_mode == RES_UP2 ? g.Wo / 2 : g.Wo;
  // ---- carve: the caller's workspace, the collapsed weight image the op's own; a route query carves nothing ----
  Arena ws(dry ? Arena::DRY : Arena::CALLER, workspace, workspace_bytes), own(dry ? Arena::DRY : Arena::OWN);
  void* xin = ws.take((size_t)batch * h * w * cpad * esz);
  void* xin1 = two ? ws.take((size_t)batch * h * w * cin1 * esz) : nullptr;
  ConvWeights wt(dtype, cout, ctot, ksize, e.wsplit, ws);
  void* yout = nhwc ? ws.take((size_t)batch * g.Ho * g.Wo * cout * esz) : (void*)y;
  void* rin = res ? ws.take((size_t)batch * Hr * Wr * cout * esz) : nullptr;
  ConvErr err(ws);
  MI355_REQUIRE(ws.ok(), -2, "conv2d_fwd: workspace too small");
  if (wants_up2_image(d, c_src0)) wt.take_up2(own);
  MI355_REQUIRE(own.ok(), -2, "conv2d_fwd: out of device memory");
  wt.describe(d, bias_host != nullptr);
  // ---- optional parts: the given prologue, the epilogue's terms, the NCHW source, the Euler update ----
  d.src0 = xin; d.src1 = xin1; d.err = err.word;
  if (pro_a) { d.pro_a = pro_a; d.pro_b = pro_b; d.pro_silu = pro_silu; }
  if (emb) { d.emb = emb; d.emb_stride = cout; }
  if (res) { d.res = rin; d.res_mode = res_mode; }
  d.out_mode = nhwc ? OUT_NHWC : OUT_NCHW_F32; d.out = ws.or_placeholder(yout);
  if (nchw_src) {
    d.nchw0 = ws.or_placeholder(x); d.nchw_c0 = cin;
    d.nchw1 = !cin1 ? nullptr : ws.or_placeholder(x1); d.nchw_c1 = cin1;
  }
  if (axpy_x) { d.axpy_x = axpy_x; d.axpy_scale = axpy_scale; }
  // ---- route (all a route query asks for), stage, launch ----
  ConvRoute r; int rc;
  if ((rc = conv_route(d, &r))) return rc;
  if (dry) { report_route(r, route, 8); return 0; }
  hipStream_t s = S(stream);
  if ((rc = err.zero(s))) return rc;
  if (!r.reads_nchw) {   // a launch that reads the caller's tensors itself leaves the packed copy as the caller filled the workspace
    if ((rc = pack_nhwc_launch(dtype, x, cin, nchw_src ? x1 : nullptr, nchw_src ? cin1 : 0, batch, h * w, cpad, xin, s))) return rc;
  }
  if (two && (rc = pack_nhwc_launch(dtype, x1, cin1, nullptr, 0, batch, h * w, cin1, xin1, s))) return rc;
  if (res && (rc = pack_nhwc_launch(dtype, res, cout, nullptr, 0, batch, Hr * Wr, cout, rin, s))) return rc;
  if ((rc = wt.stage(w_host, bias_host, s))) return rc;
  if ((rc = conv_launch(d, r, s))) return rc;
  report_route(r, route, 8);
  if (nhwc && (rc = unpack_nchw_launch(dtype, yout, batch, g.Ho * g.Wo, cout, y, s))) return rc;
  return err.finish("conv2d_fwd");
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
}  // namespace

int mi355_linear(const float* in, const float* wt, const float* bias, float* out, int batch, int k, int j, int in_act, int out_act, int32_t* form,
                 void* stream) {
  if (form) *form = -1;
  MI355_REQUIRE(in && wt && out && batch > 0 && k > 0 && j > 0, -1, "linear: bad argument");
  hipStream_t s = S(stream);
  if (int rc = linear_launch(in, wt, bias, out, batch, k, j, in_act, out_act, s)) return rc;
  if (form) *form = linear_form(batch, k);
  return synced(s);
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
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_ANY, "pack_nhwc", &e)) return rc;
  hipStream_t s = S(stream);
  if (int rc = pack_nhwc_launch(dtype, x, cx, cond, cc, batch, hw, cpad, out, s)) return rc;
  return synced(s);
}

int mi355_unpack_nchw(const void* in, int batch, int hw, int channels, float* out, int dtype, void* stream) {
  MI355_REQUIRE(in && out && batch > 0 && hw > 0 && channels > 0, -1, "unpack_nchw: bad argument");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_ANY, "unpack_nchw", &e)) return rc;
  hipStream_t s = S(stream);
  if (int rc = unpack_nchw_launch(dtype, in, batch, hw, channels, out, s)) return rc;
  return synced(s);
}

int mi355_unpack_channels(const void* in, int batch, int hw, int stride, int c0, int count, float* out, int dtype, void* stream) {
  MI355_REQUIRE(in && out && batch > 0 && hw > 0 && count > 0 && c0 >= 0, -1, "unpack_channels: bad argument");
  MI355_REQUIRE(c0 + count <= stride, -2, "unpack_channels: channels c0 .. c0 + count must lie inside a row");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_ANY, "unpack_channels", &e)) return rc;
  hipStream_t s = S(stream);
  if (int rc = unpack_channels_launch(dtype, in, batch, hw, stride, c0, count, out, s)) return rc;
  return synced(s);
}

int mi355_resample(const void* in, void* out, int batch, int h, int w, int channels, int mode, int dtype, void* stream) {
  MI355_REQUIRE(in && out && batch > 0 && h > 0 && w > 0 && channels > 0, -1, "resample: bad argument");
  MI355_REQUIRE(mode == CONV_UP2 || (mode == CONV_POOL2 && h >= 2 && w >= 2), -1, "resample: mode must be 2 (nearest x2) or 3 (2x2 average pool, h and w >= 2)");
  ElemType e; if (int rc = elem_type(&dtype, ELEMS_ANY, "resample", &e)) return rc;
  hipStream_t s = S(stream);
  if (int rc = resample_launch(dtype, in, out, batch, h, w, channels, mode, s)) return rc;
  return synced(s);
}

}  // extern "C"
