// The sampler loops of libmi355_sampler.so (see include/mi355_sampler.h): workspace layouts, the embedding rows of the evaluations, and the
// Euler (+ graph form), Runge-Kutta, DDPM, their classifier-free-guided forms, the replacement / reconstruction-guided flow sampler, and SF2M entry
// points.  Host code only.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "capi_internal.h"

// The sampler loops know every evaluation time in advance: all emb_layers outputs of up to EMB_TABLE_STEPS evaluations are computed by four
// launches before the loop instead of four launches per evaluation (longer schedules fall back to the per-evaluation path).
constexpr int EMB_TABLE_STEPS = 1024;

namespace {

// ---- workspace layouts ------------------------------------------------------------------------------
// ONE walk over the regions of a sampler's workspace: a size function walks from a null base and returns where the walk ends, a sampler walks
// from the caller's pointer and keeps the addresses.  A region's size is written here and nowhere else.
struct Walk {
  uintptr_t p;
  template <class T = float> T* take(size_t bytes) { T* r = reinterpret_cast<T*>(p); p += al256(bytes); return r; }
};
// sampler scratch: t[B], eps/v [B,32,H,W], none_like [B,32,H,W], the step times and the embedding table of EvalEmb, the graph form's resident
// state [B,Cout,H,W] (mi355_debug_config::sampler_graph), then the engine workspace
struct Scratch { float* t; float* v; float* none; float* tsteps; float* embtab; float* xstate; char* unet_ws; int64_t unet_bytes; };
// classifier-free guidance: duplicated state x | x, condition | none_value, labels | null label (the last two only where the net takes them)
struct CfgTail { float* x2; float* cond2; int32_t* labels2; };
// fixed-step Runge-Kutta: the stage derivatives k_1..k_s and the stage state y_i, each a state at the evaluation batch.  Adams-Bashforth: the ring
// of `order` stored velocities, then the start method's stages 2..s (order + s - 1 <= 7 buffers)
struct RkBufs { float* k[7]; float* ystage; };
// training-free in-painting / super-resolution of a flow (mi355_cfm_recon_sample): the call's initial state (the noise end of the straight path the
// "coupled" replacement pastes along), the seed's two outputs and the U-Net VJP, each a state; the low-res residual [B, C, h_low, w_low]
struct ReconDims { int h_low, w_low; };
struct ReconTail { float* x_init; float* g_eps; float* g_x; float* vjp; float* resid; };
// the DDPM multistep history (the previous step's data prediction: one state at `batch`, also under guidance) and the shaping rows [batch][2]
struct DdpmTail { float* hist; float* rows; };
// feature cache with drift_out: the cached feature as the previous full evaluation left it (plan element type), behind everything else
// tiled sampling (TiledEval): B canvases cut by g.  Behind everything else: the windows the net reads (x | condition: [B * nW, in_channels, S, S]),
// the windows it writes [B * nW, out_channels, S, S], the blended canvas [B, out_channels, Hc, Wc], the repeated labels [B * nW]
struct TileSpec { int B; TileGeom g; };
struct TiledTail { float* in; float* out; float* vbar; int32_t* labels; };
struct Layout { Scratch sc; CfgTail cfg; RkBufs rk; ReconTail rec; DdpmTail ddpm; void* feat_prev; TiledTail tile; uintptr_t end; };
// What a sampler call keeps in its workspace.  guided: the network runs at 2 * batch and the guidance tail follows its workspace; stages > 0: the
// Runge-Kutta buffers follow; recon: the reconstruction tail; hist, rows: the DDPM tail closes the layout.
// lv (mi355_ddpm_lv_sample): a guided net with in_channels == out_channels is a learned-variance net (state and condition of out_channels / 2 channels each).
struct LayoutSpec { int batch = 0; bool guided = false; int stages = 0; const ReconDims* recon = nullptr; bool hist = false; bool rows = false; size_t feat_bytes = 0;
                    const TileSpec* tile = nullptr; bool lv = false; };
inline size_t cfg_cond_channels(const mi355_unet* net, bool lv = false) {
  if (lv && net->cfg.in_channels == net->cfg.out_channels) return (size_t)(net->cfg.in_channels / 2);
  return (size_t)(net->cfg.in_channels > net->cfg.out_channels ? net->cfg.in_channels - net->cfg.out_channels : 0);
}

Layout layout(const mi355_unet* net, const LayoutSpec& sp, uintptr_t base) {
  const size_t hw = (size_t)net->cfg.image_size * net->cfg.image_size;
  const bool guided = sp.guided;
  const int stages = sp.stages, B = guided ? 2 * sp.batch : sp.batch;
  const ReconDims* const recon = sp.recon;
  const size_t state = (size_t)B * net->cfg.out_channels * hw * 4;
  Layout l = {};
  Walk w{base};
  l.sc.t = w.take((size_t)B * 4);
  l.sc.v = w.take((size_t)B * 32 * hw * 4);
  l.sc.none = w.take((size_t)B * 32 * hw * 4);
  l.sc.tsteps = w.take((size_t)EMB_TABLE_STEPS * 4);
  l.sc.embtab = w.take((size_t)EMB_TABLE_STEPS * ((size_t)net->emb_total + 9 * (size_t)net->cfg.model_channels) * 4);
  l.sc.xstate = w.take(state);
  l.sc.unet_bytes = unet_workspace_bytes(net, B);
  l.sc.unet_ws = reinterpret_cast<char*>(w.p);
  w.p += (size_t)l.sc.unet_bytes;   // not rounded up: mi355_unet_workspace_bytes ends here
  if (guided || stages || recon || sp.hist || sp.rows || sp.feat_bytes || sp.tile) w.p = al256(w.p);
  if (guided) {
    l.cfg.x2 = w.take(state);
    l.cfg.cond2 = w.take((size_t)B * cfg_cond_channels(net, sp.lv) * hw * 4);
    l.cfg.labels2 = w.take<int32_t>(net->num_classes > 0 ? (size_t)B * 4 : 0);
  }
  for (int i = 0; i < stages; ++i) l.rk.k[i] = w.take(state);
  if (stages > (guided ? 1 : 0)) l.rk.ystage = w.take(state);   // a one-stage guided sampler never forms a stage state (stage 1 reads the state itself)
  if (recon) {
    l.rec.x_init = w.take(state);
    l.rec.g_eps = w.take(state);
    l.rec.g_x = w.take(state);
    l.rec.vjp = w.take(state);
    l.rec.resid = w.take((size_t)B * net->cfg.out_channels * recon->h_low * recon->w_low * 4);
  }
  if (sp.hist) l.ddpm.hist = w.take((size_t)sp.batch * net->cfg.out_channels * hw * 4);
  if (sp.rows) l.ddpm.rows = w.take((size_t)sp.batch * 2 * 4);
  if (sp.feat_bytes) l.feat_prev = w.take<void>(sp.feat_bytes);
  if (sp.tile) {   // with a tile spec, sp.batch is the chunk the net runs at
    const size_t rows = (size_t)sp.tile->B * sp.tile->g.nW;
    l.tile.in = w.take(rows * net->cfg.in_channels * hw * 4);
    l.tile.out = w.take(rows * net->cfg.out_channels * hw * 4);
    l.tile.vbar = w.take((size_t)sp.tile->B * net->cfg.out_channels * sp.tile->g.Hc * sp.tile->g.Wc * 4);
    l.tile.labels = w.take<int32_t>(net->num_classes > 0 ? rows * 4 : 0);
  }
  l.end = w.p;
  return l;
}
inline int64_t layout_bytes(const mi355_unet* net, const LayoutSpec& sp) { return (int64_t)layout(net, sp, 0).end; }
inline LayoutSpec plain_spec(int batch, bool guided = false, int stages = 0) { LayoutSpec sp; sp.batch = batch; sp.guided = guided; sp.stages = stages; return sp; }

// The layout of a sampler call in the caller's workspace.  who (optional): the entry point's name in front of the short-workspace refusal.
int carve(const mi355_unet* net, const LayoutSpec& sp, void* workspace, int64_t workspace_bytes, Layout& l, const char* who = nullptr) {
  MI355_REQUIRE(net && workspace, -1, "null argument");
  MI355_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, -1, "workspace must be 256-byte aligned");
  l = layout(net, sp, reinterpret_cast<uintptr_t>(workspace));
  MI355_REQUIRE(workspace_bytes >= (int64_t)(l.end - reinterpret_cast<uintptr_t>(workspace)), -2,
                (who ? std::string(who) + ": " : std::string()) + "workspace too small");
  return 0;
}

// ---- embedding rows of the evaluations -----------------------------------------------------------------
// The emb_layers outputs of a sampler's network evaluations, whose times t_host[e] (e < n) are all known before the loop.  Where they fit, ONE
// table holds them: table[e] for an unlabelled sampler; with class labels table[e * K + c] = the rows of evaluation e and class c (three time
// launches over n rows, one label_emb_linear over n * K), from which every evaluation gathers its images' rows.  Otherwise every evaluation
// stages its time in sc.t and computes its own rows.
class EvalEmb {
 public:
  // temporary: t_host dies with the calling function, so its copy is waited for, once per call.  A caller's own array (the Euler loop, which is
  // also recorded into a graph) is not waited for; nor is one whose caller waits itself (SF2M: one wait for its two instances).
  int init(const mi355_unet* net, const Scratch& sc, const float* t_host, int64_t n, bool labelled, bool temporary, hipStream_t s) {
    sc_ = &sc; t_host_ = t_host;
    const int K = labelled ? net->num_classes : 1;
    block_ = (size_t)K * net->emb_total;
    // The rule is rows = n * K <= EMB_TABLE_STEPS (K = num_classes with labels, else 1): beyond it the table stays null and every evaluation
    // computes its own rows.  n is 64-bit so that a caller's product (steps * stages) needs no test of its own: one that left K out would only
    // keep the row count within an int and within sc.tsteps, which this rule does as well (K >= 1).
    if (n <= 0 || n * K > EMB_TABLE_STEPS) return 0;
    MI355_CHECK_HIP(hipMemcpyAsync(sc.tsteps, t_host, (size_t)n * 4, hipMemcpyHostToDevice, s));
    float* scratch = sc.embtab + (size_t)EMB_TABLE_STEPS * net->emb_total;
    if (int rc = labelled ? unet_embedding_rows_labels(net, sc.tsteps, (int)n, nullptr, (int)n * K, K, sc.embtab, scratch, s)
                          : unet_embedding_table(net, sc.tsteps, (int)n, sc.embtab, scratch, s)) return rc;
    table_ = sc.embtab;
    if (temporary) MI355_CHECK_HIP(hipStreamSynchronize(s));
    return 0;
  }
  const float* table() const { return table_; }
  // Evaluation e at `batch` images on stream s: run.emb_row = its table block, or a fill_launch of its time into sc.t (*launched: counted).
  int select(UnetRun& run, size_t e, int batch, hipStream_t s, int64_t* launched = nullptr) const {
    if (table_) { run.emb_row = table_ + e * block_; return 0; }
    if (launched) ++*launched;
    return fill_launch(sc_->t, t_host_[e], batch, s);
  }

 private:
  const Scratch* sc_ = nullptr;
  const float* t_host_ = nullptr;
  const float* table_ = nullptr;
  size_t block_ = 0;
};

// ---- classifier-free guidance: every evaluation is ONE forward at batch 2B (images 0..B-1 conditional, B..2B-1 unconditional) -------------------
// The one point where a guided loop differs from its plain form: the launch that consumes the network output.  off: the plain kernel; on: its
// guided form, which combines the two halves with w (or the per-image w_dev) over `per` elements per image.
struct Guide : StepGuide {
  int64_t per = 0;
  int stage(float* out, const float* y0, const float* const* kp, const float* cf, int nk, int64_t n, float* copy_out, uint8_t* u8_out, hipStream_t s) const {
    return on ? cfg_stage_launch(out, y0, kp, cf, nk, n, w, w_dev, per, 1, copy_out, u8_out, s) : rk_stage_launch(out, y0, kp, cf, nk, n, copy_out, u8_out, s);
  }
};
// x2 = x | x, cond2 = cond | none_value, labels2 = labels | null_label: built once per call
int cfg_fill_tail(const CfgTail& t, const float* x, int64_t n, const float* cond, int64_t nc, float none_value, const int32_t* labels, int null_label,
                  int batch, hipStream_t s) {
  MI355_CHECK_HIP(hipMemcpyAsync(t.x2, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  MI355_CHECK_HIP(hipMemcpyAsync(t.x2 + n, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  if (cond) {
    MI355_CHECK_HIP(hipMemcpyAsync(t.cond2, cond, (size_t)nc * 4, hipMemcpyDeviceToDevice, s));
    if (int rc = fill_launch(t.cond2 + nc, none_value, nc, s)) return rc;
  }
  if (labels) {
    MI355_CHECK_HIP(hipMemcpyAsync(t.labels2, labels, (size_t)batch * 4, hipMemcpyDeviceToDevice, s));
    MI355_CHECK_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(t.labels2 + batch), null_label, (size_t)batch, s));
  }
  return 0;
}

// ---- feature reuse across evaluations (DeepCache; mi355_feature_cache) -----------------------------------------------------------------
// Every refusal of a cache schedule, before any launch, each naming its argument.  n_evals: the evaluations the loop is about to make.
int check_cache(const char* who, const mi355_unet* net, const mi355_feature_cache* cache, int64_t n_evals) {
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(cache, -1, f + "cache is null");
  MI355_REQUIRE(cache->full, -1, f + "cache->full is null");
  if (unet_cache_range(net, cache->branch, nullptr, nullptr, nullptr)) {
    mi355_set_error(f + "cache->branch: " + mi355_last_error());
    return -1;
  }
  MI355_REQUIRE(!net->cfg.differentiable, -4, f + "cache: a differentiable plan cannot run shallow evaluations");
  MI355_REQUIRE((int64_t)cache->n_evals == n_evals, -1,
                f + "cache->n_evals must be the number of evaluations the loop makes (" + std::to_string(n_evals) + ", got " + std::to_string(cache->n_evals) + ")");
  MI355_REQUIRE(n_evals == 0 || cache->full[0] != 0, -1, f + "cache->full[0] must be non-zero (the first evaluation has nothing to reuse)");
  return 0;
}
// bytes of the cached feature of branch k at `batch` images (the F_prev buffer of drift_out)
size_t cache_feature_bytes(const mi355_unet* net, int k, int batch) {
  int tid = 0;
  if (unet_cache_range(net, k, nullptr, nullptr, &tid)) return 0;
  const PlanTensor& t = net->tensors[tid];
  return (size_t)t.C * t.H * t.W * (size_t)batch * (net->cfg.dtype == 0 ? 4 : 2);
}
// A loop's view of its cache schedule (a null CacheRun*: every evaluation is whole).  With drift_out, every full evaluation is followed by ONE
// launch: the first copies the cached feature into prev, the later ones are feature_drift_launch (row e of drift_out, prev <- the feature).
struct CacheRun {
  const mi355_feature_cache* cache = nullptr;
  const mi355_unet* net = nullptr;
  int tensor = -1; void* feat = nullptr; void* prev = nullptr; int64_t per = 0; int batch = 0; bool seeded = false;
  int init(const mi355_unet* n, const mi355_feature_cache* c, const Scratch& sc, void* feat_prev, int B, hipStream_t s) {
    cache = c; net = n; batch = B;
    if (!c->drift_out) return 0;
    if (int rc = unet_cache_range(n, c->branch, nullptr, nullptr, &tensor)) return rc;
    const PlanTensor& t = n->tensors[tensor];
    per = (int64_t)t.C * t.H * t.W;
    feat = WsView(n, sc.unet_ws, B).tensor(tensor); prev = feat_prev;
    return fill_launch(c->drift_out, -1.f, (int64_t)c->n_evals * B, s);   // rows of shallow evaluations and of the first full one
  }
  int branch_of(int64_t e) const { return cache->full[e] ? 0 : cache->branch; }
  int after(int64_t e, hipStream_t s) {   // evaluation e has been issued
    if (!cache->drift_out || !cache->full[e]) return 0;
    MI355_REQUIRE(net->tensor_state[tensor].load(std::memory_order_relaxed) == 0, -4, "feature cache: drift_out needs the cached feature as stored, and this forward did not materialise it");
    if (!seeded) {
      seeded = true;
      MI355_CHECK_HIP(hipMemcpyAsync(prev, feat, (size_t)per * batch * (net->cfg.dtype == 0 ? 4 : 2), hipMemcpyDeviceToDevice, s));
      return 0;
    }
    return feature_drift_launch(net->cfg.dtype, feat, prev, batch, per, cache->drift_out + e * batch, s);
  }
};

// ---- tiled evaluation (canvases larger than the net's frame; tile.hip) ----------------------------------------------------------------------
// Largest batch one forward takes: every activation tensor is addressed through 32-bit buffer offsets (the convs refuse beyond 4 GiB with "run
// the batch in slices"), and a concat source pair or an in-flight double of the same tensor halves that.  The samplers' fp32 scratch holds up to
// 32 channels per image.
int64_t net_max_batch(const mi355_unet* net) {
  const size_t esz = net->cfg.dtype == 0 ? 4 : 2;
  size_t per = (size_t)32 * net->cfg.image_size * net->cfg.image_size * 4;
  for (const PlanTensor& t : net->tensors) per = std::max(per, (size_t)t.C * t.H * t.W * (t.f32 ? 4 : esz));
  return std::max<int64_t>(1, (int64_t)(0xFFFF0000ull / (2 * per)));
}
// Every refusal of a tile plan, before any launch, each naming its field.  who: the entry point's name.
int check_tile_plan(const char* who, const mi355_unet* net, const mi355_tile_plan* plan, int batch, TileSpec& ts) {
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(net && batch > 0, -1, f + "bad argument (net, batch)");
  if (int rc = tile_geom(net->cfg.image_size, plan, &ts.g, who)) return rc;
  MI355_REQUIRE(plan->chunk <= net_max_batch(net), -1,
                f + "chunk is above the handle's largest batch (" + std::to_string(net_max_batch(net)) + ")");
  MI355_REQUIRE((int64_t)batch * ts.g.nW < (1ll << 31), -4, f + "batch * windows per canvas does not fit an int");
  ts.B = batch;
  return 0;
}
// What the loops call in place of unet_forward (a null TiledEval*: the existing path).  One evaluation = gather the state's windows, the forward on
// the windows in chunks of at most `chunk` rows (labels and condition windows sliced per chunk, no euler_x), blend: n_chunks forwards + 2 launches.
// The result is vbar (a canvas); with euler_x the blend also takes x <- x + dt * vbar.
struct TiledEval {
  TileGeom g; int B = 0, chunk = 0;
  TiledTail buf;
  const int32_t* labels = nullptr;   // null, or buf.labels once repeat_labels has run
  int64_t rows() const { return (int64_t)B * g.nW; }
  int64_t hw() const { return (int64_t)g.S * g.S; }
  float* cond_windows(int Cx) const { return buf.in + rows() * Cx * hw(); }
  // once per call: the condition canvas -> its windows (behind the state's windows), the labels [B] -> [B * nW]
  int gather_cond(const float* cond, int Cx, int Cc, hipStream_t s) const { return tile_gather_launch(cond, cond_windows(Cx), B, Cc, g, s); }
  int repeat_labels(const int32_t* lab, hipStream_t s) { labels = buf.labels; return tile_labels_launch(lab, buf.labels, B, g.nW, s); }
  // condw: null, the windows of gather_cond, or (uniform) one buffer of `chunk` rows that every chunk reads, such as the none_value fill
  int eval(const mi355_unet* net, const Scratch& sc, const UnetRun& run, const float* x, int Cx, const float* condw, int Cc, bool uniform, float* euler_x,
           float dt, hipStream_t s) const {
    if (int rc = tile_gather_launch(x, buf.in, B, Cx, g, s)) return rc;
    UnetRun r = run;
    r.euler_x = nullptr; r.euler_dt = 0.f;
    const int Cout = net->cfg.out_channels;
    int64_t launches = 2;
    for (int64_t off = 0; off < rows(); off += chunk) {
      const int m = (int)std::min<int64_t>(chunk, rows() - off);
      r.labels = labels ? labels + off : nullptr;
      const float* c = !condw ? nullptr : (uniform ? condw : condw + off * Cc * hw());
      if (int rc = unet_forward(net, buf.in + off * Cx * hw(), Cx, c, Cc, sc.t, buf.out + off * Cout * hw(), m, sc.unet_ws, sc.unet_bytes, s, r)) return rc;
      launches += net->last_launches;
    }
    if (int rc = tile_blend_launch(buf.out, buf.vbar, euler_x, dt, B, Cout, g, s)) return rc;
    net->last_launches = launches;   // mi355_unet_get_stats: every launch of the last tiled evaluation
    return 0;
  }
};
TiledEval tiled_eval(const TileSpec& ts, int chunk, const Layout& l) {
  TiledEval t;
  t.g = ts.g; t.B = ts.B; t.chunk = chunk; t.buf = l.tile;
  return t;
}

// ---- flow-matching Euler ----------------------------------------------------------------------------------
// The loop proper: every launch of every step on stream s (the caller's stream, or the handle's capture stream while a graph is recorded).
// labels: class-conditional steps (with a table: step k's block of the (step, class) table, one gather launch per step).
int cfm_euler_loop(mi355_unet* net, const Scratch& sc, const EvalEmb& emb, float* x, int x_channels, const float* cond, int cond_channels, float* cdrift,
                   const float* t_span_host, int n_t, float* traj, int batch, int64_t n, int64_t nc, hipStream_t s, const int32_t* labels = nullptr,
                   CacheRun* cache = nullptr, const TiledEval* tiled = nullptr) {
  UnetRun run = uniform_t_run();
  run.labels = labels;
  for (int k = 0; k + 1 < n_t; ++k) {
    const float dt = t_span_host[k + 1] - t_span_host[k];
    int rc;
    if ((rc = emb.select(run, (size_t)k, batch, s))) return rc;
    if (tiled) {   // x is a canvas, cond its windows, batch the chunk: the blend launch carries x += dt * vbar
      if ((rc = tiled->eval(net, sc, run, x, x_channels, cond, cond_channels, false, x, dt, s))) return rc;
      if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj + (size_t)(k + 1) * n, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      continue;
    }
    run.reuse_branch = cache ? cache->branch_of(k) : 0;   // step k is evaluation k
    run.euler_x = x; run.euler_dt = dt;   // x += dt * v: in the last conv's epilogue, or as a launch of unet_forward's own behind it
    if ((rc = unet_forward(net, x, x_channels, cond, cond_channels, sc.t, sc.v, batch, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
    if (cache && (rc = cache->after(k, s))) return rc;
    if (cdrift && (rc = euler_step_launch(cdrift, cdrift, dt, nc, s))) return rc;
    if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj + (size_t)(k + 1) * n, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

// knobs.sampler_graph: the loop as ONE graph launch.  The graph works on the workspace's resident state (sc.xstate) so that it does not depend on
// the caller's x / u8 pointers (a fresh tensor per call is the normal use); it does depend on the workspace, the batch, the schedule (dt is a kernel
// argument, the embedding rows are table addresses) and the condition pointer: those are its key.  The embedding table is rebuilt on every call,
// outside the graph (the workspace is the caller's: another sampler may have used it in between).
int cfm_euler_graph(mi355_unet* net, const Scratch& sc, const EvalEmb& emb, float* x, int x_channels, const float* cond, int cond_channels,
                    const float* t_span_host, int n_t, int batch, int64_t n, void* workspace, hipStream_t s) {
  uint64_t h = 1469598103934665603ull;
  for (int k = 0; k < n_t; ++k) { uint32_t b; std::memcpy(&b, &t_span_host[k], 4); h = (h ^ b) * 1099511628211ull; }
  const uint64_t key[8] = {(uint64_t)reinterpret_cast<uintptr_t>(workspace), (uint64_t)batch, (uint64_t)n_t, h, (uint64_t)reinterpret_cast<uintptr_t>(cond),
                           (uint64_t)cond_channels, (uint64_t)x_channels, (uint64_t)reinterpret_cast<uintptr_t>(emb.table())};
  std::lock_guard<std::mutex> lock(net->graph_mu);
  mi355_unet::SamplerGraph* g = nullptr;
  for (auto& e : net->graphs) if (e.exec && std::memcmp(e.key, key, sizeof(key)) == 0) { g = &e; break; }
  if (!g) {
    if (!net->capture_stream) MI355_CHECK_HIP(hipStreamCreateWithFlags(&net->capture_stream, hipStreamNonBlocking));
    hipStream_t cs = net->capture_stream;
    MI355_CHECK_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    int rc = cfm_euler_loop(net, sc, emb, sc.xstate, x_channels, cond, cond_channels, nullptr, t_span_host, n_t, nullptr, batch, n, 0, cs);
    hipGraph_t graph = nullptr;
    hipError_t e = hipStreamEndCapture(cs, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (e != hipSuccess || !graph) { mi355_set_error(std::string("cfm_euler_sample: graph capture failed: ") + hipGetErrorString(e)); return -3; }
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { mi355_set_error(std::string("cfm_euler_sample: graph instantiation failed: ") + hipGetErrorString(e)); return -3; }
    constexpr size_t CAP = 4;
    if (net->graphs.size() < CAP) { net->graphs.emplace_back(); g = &net->graphs.back(); }
    else {
      g = &net->graphs[0];
      for (auto& c : net->graphs) if (c.stamp < g->stamp) g = &c;
      // the replaced graph may still be running on a stream of the caller's: wait for the device before its nodes are freed (rare: a fifth key)
      (void)hipDeviceSynchronize();
      (void)hipGraphExecDestroy(g->exec);
    }
    std::memcpy(g->key, key, sizeof(key));
    g->exec = exec;
    g->launches = net->last_launches;
  }
  g->stamp = ++net->graph_clock;
  MI355_CHECK_HIP(hipMemcpyAsync(sc.xstate, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  MI355_CHECK_HIP(hipGraphLaunch(g->exec, s));
  MI355_CHECK_HIP(hipMemcpyAsync(x, sc.xstate, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  net->last_launches = g->launches;
  return 0;
}

// ---- fixed-step explicit Runge-Kutta over a general tableau (midpoint, Heun, RK4, ...) ----------------------------------------
int check_tableau(const char* who, int stages, const float* a_host, const float* b_host, const float* c_host) {
  const std::string f(who);
  MI355_REQUIRE(stages >= 1 && stages <= 4, -1, f + ": the tableau must have 1 to 4 stages");
  MI355_REQUIRE(a_host && b_host && c_host, -1, f + ": null tableau");
  bool any_b = false;
  for (int j = 0; j < stages; ++j) any_b = any_b || b_host[j] != 0.f;
  MI355_REQUIRE(any_b, -1, f + ": the tableau's weights b are all zero");
  return 0;
}
// t + c * dt with the product and the sum each rounded to fp32 (c == 0 / 1: the interval's end points themselves, as mi355/ode.py's dopri5 does)
float rk_stage_time(float t0, float t1, float c) {
#pragma clang fp contract(off)
  if (c == 0.f) return t0;
  if (c == 1.f) return t1;
  const float dt = t1 - t0;
  const float p = c * dt;
  return t0 + p;
}
// the non-zero entries of a tableau row (a stage's a_i., or b) times dt, each with its derivative buffer
int gather_row(const float* row, int count, float dt, float* const* kbuf, const float** kp, float* cf) {
  int nk = 0;
  for (int j = 0; j < count; ++j)
    if (row[j] != 0.f) { kp[nk] = kbuf[j]; cf[nk] = dt * row[j]; ++nk; }
  return nk;
}

// Adams-Bashforth over the loop below (mi355_cfm_ab_sample): steps k >= order - 1 take x_{k+1} = x_k + sum_j w[k * order + j] v_{k-j} (the step
// length inside the weight) from a ring of `order` stored velocities, v_k in slot k % order; the order - 1 steps before them are Runge-Kutta steps
// whose first stage (c_1 == 0: v(t_k, x_k) itself) goes straight into slot k.
struct AbPlan { int order; const float* w; };

// n_steps >= 1 steps of `state` (n elements per half: the whole state, or each half of a guided sampler's x | x), the network evaluated at
// batch evalB on cond / labels as given.  *step_launches: every launch of the last step (evaluations, stage launches, fill launches).
// ab (null: a Runge-Kutta step per interval): the tableau is the start method of an Adams-Bashforth sampler.
int cfm_rk_loop(mi355_unet* net, const Scratch& sc, const RkBufs& rk, const Guide& guide, float* state, int x_channels, const float* cond, int cond_channels,
                const int32_t* labels, const float* t_span_host, int n_steps, int stages, const float* a_host, const float* b_host, const float* c_host,
                float* traj, uint8_t* u8_out, int evalB, int64_t n, hipStream_t s, int64_t* step_launches, const AbPlan* ab = nullptr) {
  // every evaluation time is known in advance: one embedding row (block of num_classes rows with labels) per (step, stage), one per multistep step
  const int n_rk = ab && ab->order - 1 < n_steps ? ab->order - 1 : n_steps;
  std::vector<float> te((size_t)n_rk * stages + (size_t)(n_steps - n_rk));
  for (int k = 0; k < n_rk; ++k)
    for (int i = 0; i < stages; ++i) te[(size_t)k * stages + i] = rk_stage_time(t_span_host[k], t_span_host[k + 1], c_host[i]);
  for (int k = n_rk; k < n_steps; ++k) te[(size_t)n_rk * stages + (size_t)(k - n_rk)] = t_span_host[k];
  EvalEmb emb;
  if (int rc = emb.init(net, sc, te.data(), (int64_t)te.size(), labels != nullptr, true, s)) return rc;
  UnetRun run = uniform_t_run();   // no euler_x: the last conv stores v (conv_edge bit 3 stays out of these evaluations)
  run.labels = labels;
  const float* kp[4]; float cf[4];
  int rc = 0;
  for (int k = 0; k < n_steps; ++k) {
    const float dt = t_span_host[k + 1] - t_span_host[k];
    *step_launches = 0;
    float* const out_traj = traj ? traj + (size_t)(k + 1) * n : nullptr;
    uint8_t* const out_u8 = k + 1 == n_steps ? u8_out : nullptr;
    if (k >= n_rk) {   // one evaluation into the oldest slot, one launch over the non-zero weights (a row without one was refused)
      if ((rc = emb.select(run, (size_t)n_rk * stages + (size_t)(k - n_rk), evalB, s, step_launches))) return rc;
      if ((rc = unet_forward(net, state, x_channels, cond, cond_channels, sc.t, rk.k[k % ab->order], evalB, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
      *step_launches += net->last_launches + 1;
      int nk = 0;
      for (int j = 0; j < ab->order; ++j)
        if (const float wj = ab->w[(size_t)k * ab->order + j]; wj != 0.f) { kp[nk] = rk.k[(k - j) % ab->order]; cf[nk] = wj; ++nk; }
      if ((rc = guide.stage(state, state, kp, cf, nk, n, out_traj, out_u8, s))) return rc;
      continue;
    }
    float* kbuf[4];   // the stage derivatives: Runge-Kutta k_1..k_s; a start step: ring slot k, then the buffers behind the ring
    for (int i = 0; i < stages; ++i) kbuf[i] = !ab ? rk.k[i] : (i == 0 ? rk.k[k] : rk.k[ab->order + i - 1]);
    for (int i = 0; i < stages; ++i) {
      // y_i = state + sum_{j<i} (dt * a_ij) k_j over the non-zero a_ij; none: the stage reads the state itself
      const float* yin = state;
      if (const int nk = gather_row(a_host + (size_t)i * stages, i, dt, kbuf, kp, cf)) {
        if ((rc = guide.stage(rk.ystage, state, kp, cf, nk, n, nullptr, nullptr, s))) return rc;
        yin = rk.ystage; ++*step_launches;
      }
      if ((rc = emb.select(run, (size_t)k * stages + i, evalB, s, step_launches))) return rc;
      if ((rc = unet_forward(net, yin, x_channels, cond, cond_channels, sc.t, kbuf[i], evalB, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
      *step_launches += net->last_launches;
    }
    // the step's update, in place, with the trajectory slot and (last step) the image bytes from the same launch; nk >= 1: an all-zero b was refused
    const int nk = gather_row(b_host, stages, dt, kbuf, kp, cf);
    if ((rc = guide.stage(state, state, kp, cf, nk, n, out_traj, out_u8, s))) return rc;
    ++*step_launches;
  }
  return 0;
}

// ---- DDPM / DDIM reverse loop ----------------------------------------------------------------------------------
std::vector<float> ddpm_times(int Ns) {   // evaluation i = step i: eps_model(xi, i) = network(xi, 1.0*i/Ns)  loss_functions.py:18-19
  std::vector<float> th((size_t)(Ns > 0 ? Ns : 0));
  for (int i = 0; i < Ns; ++i) th[i] = (float)i / (float)Ns;
  return th;
}
struct DdpmLoop {
  const char* who;          // the entry point's name: prefix of the loop's refusals
  float* state; int evalB;  // the state the steps update (n elements; a guided sampler's first half) and the predictor's batch
  const float* cond_pred; const int32_t* labels_pred;   // what the net sees on predictor steps (at evalB)
  const float* cond_corr; const int32_t* labels_corr;   // ... and on corrector steps (at batch): no condition (sampling.py:116 -> none_like, the null label)
  const float* mask_cond;   // replacement mode: the condition pasted over the state
  const TiledEval* tiled;   // not null: the state is a canvas, evalB the chunk, cond_pred / cond_corr window buffers (sc.none: read by every chunk)
  float* mirror;            // guided: the state's second half, refreshed after a step's correctors
  Guide guide;
};
// What a scheduled entry point adds to the loop (mi355_ddpm_schedule, checked by check_schedule): all null = the plain descent Ns-1..0.
struct LoopSched {
  const float* ddim_sigma = nullptr;   // MI355_DDIM: sigma of step i (the DDIM(eta) step); null = the deterministic step
  const int32_t* walk = nullptr;       // levels K, ..., 0 with +-1 moves; null = K, K-1, ..., 0
  int n_walk = 0;
  const float* renoise_a = nullptr;    // an upward move L -> L+1: x <- renoise_a[L] x + renoise_b[L] z
  const float* renoise_b = nullptr;
  // MI355_DDIM, the multistep entry points: step i is the DPM-Solver++ step x <- ms_cx[i] x + ms_c0[i] D + ms_c1[i] hist, hist <- D
  const float* ms_cx = nullptr;
  const float* ms_c0 = nullptr;
  const float* ms_c1 = nullptr;
  float* hist = nullptr;               // the previous step's data prediction (n elements, behind the entry point's workspace)
  // mi355_ddpm_shaped_sample with shaping on: every predictor step is preceded by the statistics launch that fills shape [batch][2], and reads it
  const mi355_x0_shaping* shaping = nullptr;
  float* shape = nullptr;              // behind the entry point's workspace
  // mi355_ddpm_lv_sample with a learned variance range: the net writes [evalB, 2 * channels, H, W]; every consumer reads its eps channels under the image
  // stride 2 * per, and the ancestral predictor of step i > 0 is STEP_ANCESTRAL_LV with max_log[i] (min_log: the tables' clipped posterior log-variance)
  const float* lv_max_log = nullptr;
  // mi355_ddpm_sample_sched_cached: evaluation e of the loop (predictors and correctors, in loop order) is shallow where cache->full[e] == 0
  CacheRun* cache = nullptr;
  // mi355_ddpm_pred_sample: what the net's output stands for (PRED_*, ops.h); every step, the correctors and the statistics launch form x0_pre of the kind
  int pred = PRED_EPS;
  // mi355_ddpm_nullspace_sample: the predictor of step i is the null-space step (nullspace.hip) of the operator ns_op on the measurement ns_y with
  // ns_lam[i]; form 0 (the ancestral modes) with ns_sigma[i], form 1 (MI355_DDIM) with ddim_sigma[i].  wide_out: the net writes [evalB, 2 * channels,
  // H, W] and the step reads its eps channels under the image stride 2 * per (form 1 alone: no variance is read)
  const mi355_nullspace_op* ns_op = nullptr;
  const float* ns_y = nullptr;
  const float* ns_lam = nullptr;
  const float* ns_sigma = nullptr;
  bool wide_out = false;
};
// emb: row i = the evaluation of step i (ddpm_times(Ns), or a schedule's tau_i / train_steps), selected whenever step i runs, revisits included.
int ddpm_loop(mi355_unet* net, const Scratch& sc, const EvalEmb& emb, const DdpmLoop& a, const LoopSched& ls, int channels, const mi355_ddpm_tables* tb,
              const mi355_ddpm_options* opt, const float* noise, int64_t n_noise_draws, int batch, int64_t n, hipStream_t s) {
  const int mode = opt->mode, Ns = tb->Ns;
  const int64_t n_al = (n + 3) / 4 * 4;
  const int64_t sper = n / batch;   // elements per image (the shaping rows)
  float* x = a.state;
  float* const eps = a.tiled ? a.tiled->buf.vbar : sc.v;   // the network's prediction for the state
  UnetRun run = uniform_t_run(), run_corr = uniform_t_run();
  run.labels = a.labels_pred;
  run_corr.labels = a.labels_corr;
  int rc;
  int64_t draw = 0, eval = 0;
  auto next_noise = [&](const float*& zptr, int& philox, uint64_t& off) -> int {
    if (noise) {
      MI355_REQUIRE(draw < n_noise_draws, -2, std::string(a.who) + ": injected noise exhausted");
      zptr = noise + (size_t)draw * n; philox = 0; off = 0;
    } else { zptr = nullptr; philox = 1; off = (uint64_t)draw * (uint64_t)n_al; }
    ++draw;
    return 0;
  };
  // the move L -> L - 1 for i = L - 1: the replacement paste, the evaluation, the predictor, the correctors
  auto down = [&](int i) -> int {
    if (mode == MI355_DDPM_REPLACEMENT && i < (int)(Ns * opt->start_fraction)) {
      const float* z = nullptr; int ph = 0; uint64_t off = 0;
      if (opt->noise_condition && (rc = next_noise(z, ph, off))) return rc;
      if ((rc = replace_mask_launch(x, a.mask_cond, z, opt->pad_value, opt->noise_condition, tb->sqrt_alphas_cumprod[i],
                                    tb->sqrt_one_minus_alphas_cumprod[i], ph, opt->seed, off, n, s))) return rc;
    }
    if ((rc = emb.select(run, (size_t)i, a.evalB, s))) return rc;
    run_corr.emb_row = run.emb_row;
    run.reuse_branch = ls.cache ? ls.cache->branch_of(eval) : 0;
    if (a.tiled) rc = a.tiled->eval(net, sc, run, x, channels, a.cond_pred, channels, a.cond_pred == sc.none, nullptr, 0.f, s);
    else rc = unet_forward(net, x, channels, a.cond_pred, channels, sc.t, sc.v, a.evalB, sc.unet_ws, sc.unet_bytes, s, run);
    if (rc) return rc;
    if (ls.cache && (rc = ls.cache->after(eval, s))) return rc;
    ++eval;
    if (ls.ns_op) {
      NullspaceStep q;
      q.op = ls.ns_op; q.form = mode == MI355_DDIM ? 1 : 0; q.x = x; q.out = eps; q.out_stride = ls.wide_out ? 2 * sper : 0; q.y = ls.ns_y;
      q.batch = batch; q.channels = channels; q.h = q.w = net->cfg.image_size;
      q.c_recip = tb->sqrt_recip_alphas_cumprod[i]; q.c_recipm1 = tb->sqrt_recipm1_alphas_cumprod[i]; q.lam = ls.ns_lam[i]; q.seed = opt->seed;
      q.pred = ls.pred;
      if (ls.pred == PRED_V) { q.sa = tb->sqrt_alphas_cumprod[i]; q.sb = tb->sqrt_one_minus_alphas_cumprod[i]; }
      bool draws = i > 0;   // step 0 draws none in either form
      if (q.form == 1) { q.a = tb->alphas_cumprod_prev[i]; q.sigma = ls.ddim_sigma ? ls.ddim_sigma[i] : 0.f; draws = draws && ls.ddim_sigma; }
      else { q.a = tb->posterior_mean_coef1[i]; q.b = tb->posterior_mean_coef2[i]; q.sigma = ls.ns_sigma[i]; }
      if (draws && (rc = next_noise(q.z, q.use_philox, q.offset))) return rc;
      return nullspace_step_launch(q, s);
    }
    PredictorStep p;
    p.x = x; p.eps = eps; p.c_recip = tb->sqrt_recip_alphas_cumprod[i]; p.c_recipm1 = tb->sqrt_recipm1_alphas_cumprod[i];
    p.seed = opt->seed; p.guide = a.guide; p.per = sper; p.shape = ls.shape; p.n = n;
    p.eps_stride = ls.lv_max_log ? 2 * sper : 0;
    if (ls.pred == PRED_V) { p.sa = tb->sqrt_alphas_cumprod[i]; p.sb = tb->sqrt_one_minus_alphas_cumprod[i]; }
    p.pred = ls.pred;
    if (ls.shape && (rc = x0_shape_stats_launch(x, sc.v, a.guide, p.c_recip, p.c_recipm1, ls.shaping, ls.shape, nullptr, batch, sper, s, p.pred, p.sa, p.sb)))
      return rc;
    if (mode == MI355_DDIM) {
      if (ls.ms_cx) {
        p.kind = STEP_DPMPP; p.hist = ls.hist; p.a = ls.ms_cx[i]; p.b = ls.ms_c0[i]; p.c = ls.ms_c1[i];
      } else if (!ls.ddim_sigma) {
        p.kind = STEP_DDIM; p.a = tb->alphas_cumprod_prev[i];
      } else {
        p.kind = STEP_DDIM_ETA; p.a = tb->alphas_cumprod_prev[i]; p.sigma = ls.ddim_sigma[i];
        if (i > 0 && (rc = next_noise(p.z, p.use_philox, p.offset))) return rc;   // step 0 has acp_prev = 1: no noise term, no draw
      }
      return predictor_step_launch(p, s);
    }
    p.kind = STEP_ANCESTRAL; p.a = tb->posterior_mean_coef1[i]; p.b = tb->posterior_mean_coef2[i];
    if (i > 0 && (rc = next_noise(p.z, p.use_philox, p.offset))) return rc;
    if (ls.lv_max_log && i > 0) {   // step 0 draws no noise: the plain step, which never reads v
      p.kind = STEP_ANCESTRAL_LV; p.min_log = tb->posterior_log_variance_clipped[i]; p.max_log = ls.lv_max_log[i];
    } else {
      p.sigma = expf(0.5f * tb->posterior_log_variance_clipped[i]);
    }
    if ((rc = predictor_step_launch(p, s))) return rc;
    for (int c = 0; c < opt->n_corrector; ++c) {   // at batch B (a guided sampler's first half)
      run_corr.reuse_branch = ls.cache ? ls.cache->branch_of(eval) : 0;
      if (a.tiled) rc = a.tiled->eval(net, sc, run_corr, x, channels, a.cond_corr, channels, true, nullptr, 0.f, s);
      else rc = unet_forward(net, x, channels, a.cond_corr, channels, sc.t, sc.v, batch, sc.unet_ws, sc.unet_bytes, s, run_corr);
      if (rc) return rc;
      if (ls.cache && (rc = ls.cache->after(eval, s))) return rc;
      ++eval;
      const float* z2 = nullptr; int ph2 = 0; uint64_t off2 = 0;
      if ((rc = next_noise(z2, ph2, off2))) return rc;
      const float dt = (opt->tmax - opt->tmin) / (float)Ns;
      if ((rc = corrector_step_launch(x, eps, z2, tb->sqrt_recip_alphas_cumprod[i], tb->sqrt_recipm1_alphas_cumprod[i],
                                      tb->recip_sqrt_m1_alphas_cumprod[i], dt, opt->delta, ph2, opt->seed, off2, n, s, sper, p.eps_stride, p.pred, p.sa, p.sb)))
        return rc;
    }
    if (a.mirror && opt->n_corrector > 0) MI355_CHECK_HIP(hipMemcpyAsync(a.mirror, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return 0;
  };
  if (!ls.walk) {
    for (int i = Ns - 1; i >= 0; --i) if ((rc = down(i))) return rc;
  } else {
    for (int j = 0; j + 1 < ls.n_walk; ++j) {
      const int L = ls.walk[j];
      if (ls.walk[j + 1] < L) { if ((rc = down(L - 1))) return rc; continue; }
      const float* z = nullptr; int ph = 0; uint64_t off = 0;   // L -> L + 1: q(x_L | x_{L-1}), one draw
      if ((rc = next_noise(z, ph, off))) return rc;
      if ((rc = renoise_step_launch(x, z, ls.renoise_a[L], ls.renoise_b[L], ph, opt->seed, off, n, s))) return rc;
    }
  }
  return clip_launch(x, -1.f, 1.f, n, s);
}

// Every refusal of a mi355_ddpm_schedule, before any launch, each naming its argument.
int check_schedule(const char* who, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sd, bool guided, LoopSched& ls) {
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(sd, -1, f + "sched is null");
  const int K = tb->Ns;
  MI355_REQUIRE(sd->train_steps >= 1, -1, f + "train_steps must be >= 1");
  MI355_REQUIRE(sd->steps || K <= 0, -1, f + "steps is null");
  for (int k = 0; k < K; ++k)
    MI355_REQUIRE(sd->steps[k] >= 0 && sd->steps[k] < sd->train_steps && (k == 0 || sd->steps[k] > sd->steps[k - 1]), -1,
                  f + "steps must be strictly increasing training indices in [0, train_steps)");
  MI355_REQUIRE(!sd->ddim_sigma || opt->mode == MI355_DDIM, -1, f + "ddim_sigma belongs to MI355_DDIM (the other modes take their variance from the tables)");
  for (int k = 0; sd->ddim_sigma && k < K; ++k)
    MI355_REQUIRE(sd->ddim_sigma[k] >= 0.f && sd->ddim_sigma[k] <= 3.0e38f, -1, f + "ddim_sigma must be finite and >= 0");
  ls = LoopSched();
  ls.ddim_sigma = sd->ddim_sigma;
  if (!sd->walk) return 0;
  MI355_REQUIRE(sd->n_walk >= 1 && sd->walk[0] == K, -1, f + "walk must start at level K (= tables->Ns)");
  MI355_REQUIRE(sd->walk[sd->n_walk - 1] == 0, -1, f + "walk must end at level 0");
  bool up = false;
  for (int j = 0; j + 1 < sd->n_walk; ++j) {
    const int64_t d = (int64_t)sd->walk[j + 1] - (int64_t)sd->walk[j];
    MI355_REQUIRE((d == 1 || d == -1) && sd->walk[j + 1] >= 0 && sd->walk[j + 1] <= K, -1, f + "walk must move by +-1 between levels in [0, K]");
    up = up || d == 1;
  }
  MI355_REQUIRE(!up || !guided, -1, f + "walk has upward moves: the guided sampler's mirror half is not built for re-noising");
  MI355_REQUIRE(!up || (sd->renoise_a && sd->renoise_b), -1, f + "walk has upward moves: renoise_a and renoise_b are needed");
  ls.walk = sd->walk; ls.n_walk = sd->n_walk; ls.renoise_a = sd->renoise_a; ls.renoise_b = sd->renoise_b;
  return 0;
}
// Every refusal of a mi355_multistep_schedule, before any launch, each naming its argument; sd: its steps as a mi355_ddpm_schedule (for sched_times).
int check_multistep(const char* who, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const mi355_multistep_schedule* ms, bool guided,
                    mi355_ddpm_schedule& sd, LoopSched& ls) {
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(ms, -1, f + "msched is null");
  MI355_REQUIRE(opt->mode == MI355_DDIM, -1, f + "opt->mode must be MI355_DDIM (the multistep solver is deterministic and works on the DDIM form)");
  sd = mi355_ddpm_schedule();
  sd.steps = ms->steps; sd.train_steps = ms->train_steps;
  if (int rc = check_schedule(who, tb, opt, &sd, guided, ls)) return rc;
  const int K = tb->Ns;
  MI355_REQUIRE(K <= 0 || ms->cx, -1, f + "cx is null");
  MI355_REQUIRE(K <= 0 || ms->c0, -1, f + "c0 is null");
  MI355_REQUIRE(K <= 0 || ms->c1, -1, f + "c1 is null");
  for (int k = 0; k < K; ++k) {
    MI355_REQUIRE(std::isfinite(ms->cx[k]), -1, f + "cx must be finite");
    MI355_REQUIRE(std::isfinite(ms->c0[k]), -1, f + "c0 must be finite");
    MI355_REQUIRE(std::isfinite(ms->c1[k]), -1, f + "c1 must be finite");
  }
  MI355_REQUIRE(K <= 0 || ms->c1[K - 1] == 0.f, -1, f + "c1[K-1] must be 0: the first step run has no history to read");
  ls.ms_cx = ms->cx; ls.ms_c0 = ms->c0; ls.ms_c1 = ms->c1;
  return 0;
}
std::vector<float> sched_times(int K, const mi355_ddpm_schedule* sd) {   // evaluation k = step k: network(x, (float)tau_k / (float)train_steps)
  std::vector<float> th((size_t)(K > 0 ? K : 0));
  for (int k = 0; k < K; ++k) th[k] = (float)sd->steps[k] / (float)sd->train_steps;
  return th;
}

// The evaluations ddpm_loop makes: one per downward move, and n_corrector more behind each ancestral predictor (the DDIM steps have no corrector).
int64_t ddpm_eval_count(const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const LoopSched& ls) {
  int64_t down = tb->Ns > 0 ? tb->Ns : 0;
  if (ls.walk) {
    down = 0;
    for (int j = 0; j + 1 < ls.n_walk; ++j) down += ls.walk[j + 1] < ls.walk[j];
  }
  return down * (1 + (opt->mode == MI355_DDIM ? 0 : (int64_t)(opt->n_corrector > 0 ? opt->n_corrector : 0)));
}

// One DDPM call: the seven entry points check their own arguments, fill this, and run ddpm_run.
struct DdpmGuidance { const int32_t* labels; int null_label; float w; const float* w_dev; };
struct DdpmCall {
  const char* who;                  // the entry point's name: prefix of the refusals
  const DdpmGuidance* guided;       // null: the plain loop
  std::vector<float> th;            // the K evaluation times
  LoopSched ls;                     // what the schedule adds; hist and shape are placed by ddpm_run
  LayoutSpec spec;                  // batch, guided, the DDPM tail
  bool bare_size_refusal = false;   // mi355_ddpm_sample(_sched): their short-workspace refusal carries no prefix
  bool count_step = false;          // mi355_unet_get_stats: the last evaluation AND the launches of its step (the multistep and shaped entry points)
  const mi355_feature_cache* cache = nullptr;   // mi355_ddpm_sample_sched_cached (checked by check_cache)
  const TileSpec* tile = nullptr;   // mi355_ddpm_sample_tiled (checked by check_tile_plan): x, cond and noise are canvases, spec.batch is the chunk
  const int32_t* labels = nullptr;  // mi355_ddpm_nullspace_sample: class labels of the plain (unguided, untiled) loop
};
DdpmCall ddpm_call(const char* who, int batch, const DdpmGuidance* guided) {
  DdpmCall c = {};
  c.who = who; c.guided = guided; c.spec.batch = batch; c.spec.guided = guided != nullptr;
  return c;
}

int ddpm_run(DdpmCall& c, mi355_unet* net, float* x, int channels, const float* cond, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt,
             const float* noise, int64_t n_noise_draws, void* workspace, int64_t workspace_bytes, void* stream) {
  const std::string f = std::string(c.who) + ": ";
  const DdpmGuidance* const g = c.guided;
  const int mode = opt->mode, batch = c.tile ? c.tile->B : c.spec.batch;
  const bool amortized = net->cfg.in_channels == 2 * channels;
  const bool learned = c.ls.lv_max_log != nullptr;
  const char* const width = learned ? "var->learned needs a net whose out_channels == 2 * channels (eps and the variance channels)"
                                    : "eps model must output the state's channel count";
  const int eps_channels = learned || c.ls.wide_out ? 2 * channels : channels;
  if (g) {
    const int32_t* const labels = g->labels; const int null_label = g->null_label;
    MI355_REQUIRE(mode == MI355_DDPM_AMORTIZED || mode == MI355_DDIM, -1,
                  f + "guidance is built for the amortized sampler and for DDIM with a condition (prior and replacement modes are refused)");
    MI355_REQUIRE(cond || labels, -1, f + "nothing to guide (neither a condition nor class labels)");
    MI355_REQUIRE(!labels || net->num_classes > 0, -1, f + "class labels given to a net built without num_classes");
    MI355_REQUIRE(!labels || (null_label >= 0 && null_label < net->num_classes), -1, f + "null_label must be a class index in [0, num_classes)");
    MI355_REQUIRE(eps_channels == net->cfg.out_channels, -2, f + width);
    MI355_REQUIRE(net->cfg.in_channels == 2 * channels && cond, -2, f + "needs a 2C-input net and a condition");
  } else {
    MI355_REQUIRE(eps_channels == net->cfg.out_channels, -2, f + width);
    MI355_REQUIRE(amortized || net->cfg.in_channels == channels, -2, f + "network in_channels must be C or 2C");
    MI355_REQUIRE(mode != MI355_DDPM_REPLACEMENT || (!amortized && cond), -2, f + "replacement needs an unconditional net and a condition");
    MI355_REQUIRE(mode != MI355_DDPM_AMORTIZED || (amortized && cond), -2, f + "amortized needs a 2C-input net and a condition");
  }
  Layout l;
  if (int rc = carve(net, c.spec, workspace, workspace_bytes, l, c.bare_size_refusal ? nullptr : c.who)) return rc;
  const Scratch& sc = l.sc;
  const CfgTail& tl = l.cfg;
  c.ls.hist = l.ddpm.hist; c.ls.shape = c.ls.shaping ? l.ddpm.rows : nullptr;
  hipStream_t s = S(stream);
  const int64_t hw = c.tile ? (int64_t)c.tile->g.Hc * c.tile->g.Wc : (int64_t)net->cfg.image_size * net->cfg.image_size;
  const int64_t per = (int64_t)channels * hw, n = (int64_t)batch * per;
  EvalEmb emb;   // row i (block of num_classes rows with labels) = step i
  if (int rc = emb.init(net, sc, c.th.data(), tb->Ns, (g && g->labels) || c.labels, true, s)) return rc;
  DdpmLoop a = {};
  a.who = c.who;
  TiledEval te;
  if (g) {
    if (int rc = cfg_fill_tail(tl, x, n, cond, n, opt->none_value, g->labels, g->null_label, batch, s)) return rc;
    a.state = tl.x2; a.evalB = 2 * batch; a.mirror = tl.x2 + n;
    a.cond_pred = tl.cond2; a.labels_pred = g->labels ? tl.labels2 : nullptr;
    a.cond_corr = tl.cond2 + n; a.labels_corr = g->labels ? tl.labels2 + batch : nullptr;
    a.guide.on = true; a.guide.w = g->w; a.guide.w_dev = g->w_dev; a.guide.per = per;
  } else if (c.tile) {
    // the loop below on canvases: the condition the net sees becomes its windows (gathered once), the none_value condition one chunk-sized fill
    te = tiled_eval(*c.tile, c.spec.batch, l);
    const int64_t whw = (int64_t)net->cfg.image_size * net->cfg.image_size;
    if (amortized) { if (int rc = fill_launch(sc.none, opt->none_value, (int64_t)c.spec.batch * channels * whw, s)) return rc; }
    const bool sees_cond = amortized && (mode == MI355_DDPM_AMORTIZED || (mode == MI355_DDIM && cond));
    if (sees_cond) { if (int rc = te.gather_cond(cond, channels, channels, s)) return rc; }
    a.state = x; a.evalB = c.spec.batch; a.mask_cond = cond; a.tiled = &te;
    a.cond_pred = !amortized ? nullptr : (sees_cond ? te.cond_windows(channels) : sc.none);
    a.cond_corr = amortized ? sc.none : nullptr;
  } else {
    if (amortized) { if (int rc = fill_launch(sc.none, opt->none_value, n, s)) return rc; }
    a.state = x; a.evalB = batch; a.mask_cond = cond; a.labels_pred = c.labels;
    // the net's condition input on predictor steps / on corrector steps (the reference's corrector calls
    // x0_model without the condition, sampling.py:116 -> none_like)
    a.cond_pred = !amortized ? nullptr : ((mode == MI355_DDPM_AMORTIZED || (mode == MI355_DDIM && cond)) ? cond : sc.none);
    a.cond_corr = amortized ? sc.none : nullptr;
  }
  CacheRun cr;
  if (c.cache) {
    if (int rc = cr.init(net, c.cache, sc, l.feat_prev, batch, s)) return rc;
    c.ls.cache = &cr;
  }
  if (int rc = ddpm_loop(net, sc, emb, a, c.ls, channels, tb, opt, noise, n_noise_draws, batch, n, s)) return rc;
  if (g) MI355_CHECK_HIP(hipMemcpyAsync(x, tl.x2, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  // after the loop last_launches is the last evaluation's count; with count_step the launches of its step join it: the step launch, and the
  // statistics launch in front of it where shaping is on
  if (c.count_step && tb->Ns > 0) net->last_launches += c.ls.shape ? 2 : 1;
  return 0;
}

// ---- the fixed-step flow samplers: Runge-Kutta and Adams-Bashforth, plain and guided -----------------------------------------------------------
// One body behind mi355_cfm_rk_sample, mi355_cfm_cfg_sample, mi355_cfm_ab_sample and mi355_cfm_ab_cfg_sample, run after the entry point's own
// no-handle checks, which fill a CfmCall; the other arguments are the entry point's own.
struct CfmGuidance { float none_value; int null_label; float w; const float* w_dev; };
struct CfmCall {
  const char* who;                       // the entry point's name: prefix of the refusals
  int stages; const float* a_host; const float* b_host; const float* c_host;   // the tableau; with ab, its start method
  const CfmGuidance* guided = nullptr;   // null: the plain loop
  const AbPlan* ab = nullptr;            // null: a Runge-Kutta step per interval
  bool report_launches = true;           // mi355_unet_get_stats: every launch of the last step (evaluations and stage launches)
};
int cfm_fixed_run(const CfmCall& c, mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, const int32_t* labels,
                  const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  const std::string f = std::string(c.who) + ": ";
  const CfmGuidance* const g = c.guided;
  const AbPlan* const ab = c.ab;
  const int stages = c.stages;
  if (g) MI355_REQUIRE(cond || labels, -1, f + "nothing to guide (neither a condition nor class labels)");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, f + "class labels given to a net built without num_classes");
  if (g) {
    const int null_label = g->null_label;
    MI355_REQUIRE(!labels || (null_label >= 0 && null_label < net->num_classes), -1, f + "null_label must be a class index in [0, num_classes)");
  }
  MI355_REQUIRE(x_channels == net->cfg.out_channels, -2, f + "the vector field must have the state's channel count");
  if (g)
    MI355_REQUIRE(!cond || (cond_channels > 0 && (size_t)cond_channels == cfg_cond_channels(net)), -2,
                  f + "the condition must have in_channels - out_channels channels");
  Layout l;
  if (int rc = carve(net, plain_spec(batch, g != nullptr, ab ? ab->order + stages - 1 : stages), workspace, workspace_bytes, l, c.who)) return rc;
  const CfgTail& tl = l.cfg;
  hipStream_t s = S(stream);
  const int64_t hw = (int64_t)net->cfg.image_size * net->cfg.image_size;
  const int64_t per = (int64_t)x_channels * hw, n = (int64_t)batch * per, nc = (int64_t)batch * cond_channels * hw;
  if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  if (n_t == 1) return u8_out ? quantize_u8_launch(x, u8_out, n, s) : 0;
  Guide guide;
  float* state = x;
  if (g) {   // the loop runs on x | x at twice the batch, on cond | none_value and labels | null_label
    if (int rc = cfg_fill_tail(tl, x, n, cond, nc, g->none_value, labels, g->null_label, batch, s)) return rc;
    guide.on = true; guide.w = g->w; guide.w_dev = g->w_dev; guide.per = per;
    state = tl.x2; cond = cond ? tl.cond2 : nullptr; labels = labels ? tl.labels2 : nullptr;
  }
  int64_t step_launches = 0;
  if (int rc = cfm_rk_loop(net, l.sc, l.rk, guide, state, x_channels, cond, cond_channels, labels, t_span_host, n_t - 1, stages, c.a_host, c.b_host, c.c_host,
                           traj, u8_out, g ? 2 * batch : batch, n, s, &step_launches, ab)) return rc;
  if (g) MI355_CHECK_HIP(hipMemcpyAsync(x, tl.x2, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  if (c.report_launches) net->last_launches = step_launches;
  return 0;
}

}  // namespace

extern "C" {

int64_t mi355_unet_workspace_bytes(const mi355_unet* net, int batch) {
  if (!net || batch <= 0) { mi355_set_error("bad argument"); return -1; }
  return layout_bytes(net, plain_spec(batch));
}

int64_t mi355_cfm_rk_workspace_bytes(const mi355_unet* net, int batch, int stages) {
  if (!net || batch <= 0 || stages < 1 || stages > 4) { mi355_set_error("cfm_rk_workspace_bytes: bad argument (1 <= stages <= 4)"); return -1; }
  return layout_bytes(net, plain_spec(batch, false, stages));
}

int64_t mi355_cfg_workspace_bytes(const mi355_unet* net, int batch, int stages) {
  if (!net || batch <= 0 || stages < 1 || stages > 4) { mi355_set_error("cfg_workspace_bytes: bad argument (1 <= stages <= 4)"); return -1; }
  return layout_bytes(net, plain_spec(batch, true, stages));
}

int64_t mi355_ddpm_cfg_workspace_bytes(const mi355_unet* net, int batch) {
  if (!net || batch <= 0) { mi355_set_error("ddpm_cfg_workspace_bytes: bad argument"); return -1; }
  return layout_bytes(net, plain_spec(batch, true));
}

int64_t mi355_feature_cache_workspace_bytes(const mi355_unet* net, int batch, int branch, int drift) {
  if (!net || batch <= 0) { mi355_set_error("feature_cache_workspace_bytes: bad argument"); return -1; }
  if (unet_cache_range(net, branch, nullptr, nullptr, nullptr)) { mi355_set_error(std::string("feature_cache_workspace_bytes: branch: ") + mi355_last_error()); return -1; }
  LayoutSpec sp = plain_spec(batch);
  if (drift) sp.feat_bytes = cache_feature_bytes(net, branch, batch);
  return (int64_t)al256((size_t)layout_bytes(net, sp));
}

int mi355_cfm_euler_sample(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, int cond_drift,
                           const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  return mi355_cfm_euler_sample_labels(net, x, x_channels, cond, cond_channels, cond_drift, nullptr, t_span_host, n_t, traj, u8_out, batch,
                                       workspace, workspace_bytes, stream);
}

// mi355_cfm_euler_sample_labels and mi355_cfm_euler_sample_cached: one body, cache null for the first
static int cfm_euler_run(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, int cond_drift, const int32_t* labels,
                         const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch, void* workspace, int64_t workspace_bytes, void* stream,
                         const mi355_feature_cache* cache);

int mi355_cfm_euler_sample_labels(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, int cond_drift,
                                  const int32_t* labels, const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  return cfm_euler_run(net, x, x_channels, cond, cond_channels, cond_drift, labels, t_span_host, n_t, traj, u8_out, batch, workspace, workspace_bytes, stream,
                       nullptr);
}

int mi355_cfm_euler_sample_cached(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, int cond_drift,
                                  const int32_t* labels, const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch,
                                  void* workspace, int64_t workspace_bytes, void* stream, const mi355_feature_cache* cache) {
  MI355_REQUIRE(net && x && t_span_host && n_t >= 1, -1, "cfm_euler_sample_cached: bad argument");
  if (int rc = check_cache("cfm_euler_sample_cached", net, cache, (int64_t)n_t - 1)) return rc;
  return cfm_euler_run(net, x, x_channels, cond, cond_channels, cond_drift, labels, t_span_host, n_t, traj, u8_out, batch, workspace, workspace_bytes, stream,
                       cache);
}

static int cfm_euler_run(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, int cond_drift, const int32_t* labels,
                         const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch, void* workspace, int64_t workspace_bytes, void* stream,
                         const mi355_feature_cache* cache) {
  MI355_REQUIRE(net && x && t_span_host && n_t >= 1, -1, "cfm_euler_sample: bad argument");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "cfm_euler_sample: class labels given to a net built without num_classes");
  MI355_REQUIRE(x_channels == net->cfg.out_channels, -2, "cfm_euler_sample: the vector field must have the state's channel count");
  Layout l;
  LayoutSpec spec = plain_spec(batch);
  if (cache && cache->drift_out) spec.feat_bytes = cache_feature_bytes(net, cache->branch, batch);
  if (int rc = carve(net, spec, workspace, workspace_bytes, l)) return rc;
  const Scratch& sc = l.sc;
  hipStream_t s = S(stream);
  CacheRun cr;
  if (cache) { if (int rc = cr.init(net, cache, sc, l.feat_prev, batch, s)) return rc; }
  EvalEmb emb;   // t_span_host is the caller's array: no wait
  if (int rc = emb.init(net, sc, t_span_host, n_t - 1, labels != nullptr, false, s)) return rc;
  const int64_t n = (int64_t)batch * x_channels * net->cfg.image_size * net->cfg.image_size;
  const int64_t nc = (int64_t)batch * cond_channels * net->cfg.image_size * net->cfg.image_size;
  if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  // cond_drift: the reference integrates the CONCATENATED state [x, con] whose second half has derivative con itself
  // (mnist/utils_mnist2.py:120-124), so under Euler the condition the model sees is con_{k+1} = con_k + dt * con_k.
  // The drifting copy lives in the sampler scratch (the caller's tensor is not modified).
  float* cdrift = nullptr;
  if (cond && cond_drift) {
    MI355_REQUIRE(cond_channels <= 32, -2, "cfm_euler_sample: condition has more than 32 channels");
    cdrift = sc.none;
    MI355_CHECK_HIP(hipMemcpyAsync(cdrift, cond, (size_t)nc * 4, hipMemcpyDeviceToDevice, s));
    cond = cdrift;
  }
  int rc;
  if (net->knobs.sampler_graph && emb.table() && !traj && !cdrift && !labels && !cache && n_t > 1)
    rc = cfm_euler_graph(net, sc, emb, x, x_channels, cond, cond_channels, t_span_host, n_t, batch, n, workspace, s);
  else
    rc = cfm_euler_loop(net, sc, emb, x, x_channels, cond, cond_channels, cdrift, t_span_host, n_t, traj, batch, n, nc, s, labels, cache ? &cr : nullptr);
  if (rc) return rc;
  if (u8_out) return quantize_u8_launch(x, u8_out, n, s);
  return 0;
}

// Runge-Kutta entry points: the handle checks run first, check_tableau behind them.
int mi355_cfm_rk_sample(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, const int32_t* labels,
                        const float* t_span_host, int n_t, int stages, const float* a_host, const float* b_host, const float* c_host, float* traj,
                        uint8_t* u8_out, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && t_span_host && n_t >= 1 && batch > 0, -1, "cfm_rk_sample: bad argument");
  if (int rc = check_tableau("cfm_rk_sample", stages, a_host, b_host, c_host)) return rc;
  CfmCall c{"cfm_rk_sample", stages, a_host, b_host, c_host};
  c.report_launches = false;   // this entry point alone: mi355_unet_get_stats keeps the last evaluation's count after it
  return cfm_fixed_run(c, net, x, x_channels, cond, cond_channels, labels, t_span_host, n_t, traj, u8_out, batch, workspace, workspace_bytes, stream);
}

int mi355_cfm_cfg_sample(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, float none_value, const int32_t* labels,
                         int null_label, float w, const float* w_dev, const float* t_span_host, int n_t, int stages, const float* a_host,
                         const float* b_host, const float* c_host, float* traj, uint8_t* u8_out, int batch, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  MI355_REQUIRE(net && x && t_span_host && n_t >= 1 && batch > 0, -1, "cfm_cfg_sample: bad argument");
  if (int rc = check_tableau("cfm_cfg_sample", stages, a_host, b_host, c_host)) return rc;
  const CfmGuidance g{none_value, null_label, w, w_dev};
  CfmCall c{"cfm_cfg_sample", stages, a_host, b_host, c_host};
  c.guided = &g;
  return cfm_fixed_run(c, net, x, x_channels, cond, cond_channels, labels, t_span_host, n_t, traj, u8_out, batch, workspace, workspace_bytes, stream);
}

int mi355_ddpm_sample(mi355_unet* net, float* x, int channels, const float* cond, const mi355_ddpm_tables* tb,
                      const mi355_ddpm_options* opt, const float* noise, int64_t n_noise_draws, int batch, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && tb && opt, -1, "ddpm_sample: null argument");
  DdpmCall c = ddpm_call("ddpm_sample", batch, nullptr);
  c.th = ddpm_times(tb->Ns); c.bare_size_refusal = true;
  return ddpm_run(c, net, x, channels, cond, tb, opt, noise, n_noise_draws, workspace, workspace_bytes, stream);
}

int mi355_ddpm_sample_sched(mi355_unet* net, float* x, int channels, const float* cond, const mi355_ddpm_tables* tb,
                            const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sched, const float* noise, int64_t n_noise_draws, int batch,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && tb && opt, -1, "ddpm_sample_sched: null argument");
  DdpmCall c = ddpm_call("ddpm_sample_sched", batch, nullptr);
  if (int rc = check_schedule(c.who, tb, opt, sched, false, c.ls)) return rc;
  c.th = sched_times(tb->Ns, sched); c.bare_size_refusal = true;
  return ddpm_run(c, net, x, channels, cond, tb, opt, noise, n_noise_draws, workspace, workspace_bytes, stream);
}

int mi355_ddpm_sample_sched_cached(mi355_unet* net, float* x, int channels, const float* cond, const mi355_ddpm_tables* tb,
                                   const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sched, const float* noise, int64_t n_noise_draws, int batch,
                                   void* workspace, int64_t workspace_bytes, void* stream, const mi355_feature_cache* cache) {
  MI355_REQUIRE(net && x && tb && opt, -1, "ddpm_sample_sched_cached: null argument");
  DdpmCall c = ddpm_call("ddpm_sample_sched_cached", batch, nullptr);
  if (int rc = check_schedule(c.who, tb, opt, sched, false, c.ls)) return rc;
  if (int rc = check_cache(c.who, net, cache, ddpm_eval_count(tb, opt, c.ls))) return rc;
  c.cache = cache;
  if (cache->drift_out) c.spec.feat_bytes = cache_feature_bytes(net, cache->branch, batch);
  c.th = sched_times(tb->Ns, sched); c.bare_size_refusal = true;
  return ddpm_run(c, net, x, channels, cond, tb, opt, noise, n_noise_draws, workspace, workspace_bytes, stream);
}

int mi355_ddpm_cfg_sample(mi355_unet* net, float* x, int channels, const float* cond, const int32_t* labels, int null_label, float w, const float* w_dev,
                          const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const float* noise, int64_t n_noise_draws, int batch,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && tb && opt && batch > 0, -1, "ddpm_cfg_sample: bad argument");
  const DdpmGuidance g{labels, null_label, w, w_dev};
  DdpmCall c = ddpm_call("ddpm_cfg_sample", batch, &g);
  c.th = ddpm_times(tb->Ns);
  return ddpm_run(c, net, x, channels, cond, tb, opt, noise, n_noise_draws, workspace, workspace_bytes, stream);
}

int mi355_ddpm_cfg_sample_sched(mi355_unet* net, float* x, int channels, const float* cond, const int32_t* labels, int null_label, float w,
                                const float* w_dev, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sched,
                                const float* noise, int64_t n_noise_draws, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && tb && opt && batch > 0, -1, "ddpm_cfg_sample_sched: bad argument");
  const DdpmGuidance g{labels, null_label, w, w_dev};
  DdpmCall c = ddpm_call("ddpm_cfg_sample_sched", batch, &g);
  if (int rc = check_schedule(c.who, tb, opt, sched, true, c.ls)) return rc;
  c.th = sched_times(tb->Ns, sched);
  return ddpm_run(c, net, x, channels, cond, tb, opt, noise, n_noise_draws, workspace, workspace_bytes, stream);
}

// The multistep entry points keep the history, one state at `batch`, behind the unscheduled entry point's workspace.
int64_t mi355_ddpm_multistep_workspace_bytes(const mi355_unet* net, int batch, int guided) {
  if (!net || batch <= 0) { mi355_set_error("ddpm_multistep_workspace_bytes: bad argument"); return -1; }
  LayoutSpec sp = plain_spec(batch, guided != 0);
  sp.hist = true;
  return layout_bytes(net, sp);
}

int mi355_ddpm_multistep_sample(mi355_unet* net, float* x, int channels, const float* cond, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt,
                                const mi355_multistep_schedule* msched, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(tb && opt, -1, "ddpm_multistep_sample: tables or opt is null");
  DdpmCall c = ddpm_call("ddpm_multistep_sample", batch, nullptr);
  mi355_ddpm_schedule sd;   // the schedule's refusals need no handle
  if (int rc = check_multistep(c.who, tb, opt, msched, false, sd, c.ls)) return rc;
  MI355_REQUIRE(net && x && workspace && batch > 0, -1, "ddpm_multistep_sample: bad argument (net, x, workspace, batch)");
  c.th = sched_times(tb->Ns, &sd); c.spec.hist = true; c.count_step = true;
  return ddpm_run(c, net, x, channels, cond, tb, opt, nullptr, 0, workspace, workspace_bytes, stream);
}

int mi355_ddpm_multistep_cfg_sample(mi355_unet* net, float* x, int channels, const float* cond, const int32_t* labels, int null_label, float w,
                                    const float* w_dev, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt,
                                    const mi355_multistep_schedule* msched, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(tb && opt, -1, "ddpm_multistep_cfg_sample: tables or opt is null");
  const DdpmGuidance g{labels, null_label, w, w_dev};
  DdpmCall c = ddpm_call("ddpm_multistep_cfg_sample", batch, &g);
  mi355_ddpm_schedule sd;
  if (int rc = check_multistep(c.who, tb, opt, msched, true, sd, c.ls)) return rc;
  MI355_REQUIRE(net && x && workspace && batch > 0, -1, "ddpm_multistep_cfg_sample: bad argument (net, x, workspace, batch)");
  c.th = sched_times(tb->Ns, &sd); c.spec.hist = true; c.count_step = true;
  return ddpm_run(c, net, x, channels, cond, tb, opt, nullptr, 0, workspace, workspace_bytes, stream);
}

// Per-image shaping of the data prediction (mi355_x0_shaping): one entry point over the six loops above.  The rows (f, s) of the images close the
// workspace of the loop chosen (kept in the layout whether or not shaping is on: the size does not depend on the shaping).
int64_t mi355_ddpm_shaped_workspace_bytes(const mi355_unet* net, int batch, int guided, int multistep) {
  if (!net || batch <= 0) { mi355_set_error("ddpm_shaped_workspace_bytes: bad argument"); return -1; }
  LayoutSpec sp = plain_spec(batch, guided != 0);
  sp.hist = multistep != 0; sp.rows = true;
  return layout_bytes(net, sp);
}

// The entry points that sit over the six loops - mi355_ddpm_shaped_sample (rows), mi355_ddpm_lv_sample (lv), mi355_ddpm_pred_sample (both) - are ONE body:
// the refusals that need no handle in the order each entry point always had (its own struct's, then the schedule's), under its name, then ddpm_run.
struct OverLoops {
  const char* who; bool rows, lv;
  const mi355_ddpm_variance* var; const mi355_x0_shaping* shaping; const mi355_ddpm_prediction* pred;
};
static int ddpm_over_loops(const OverLoops& o, mi355_unet* net, float* x, int channels, const float* cond, const int32_t* labels, int null_label, int guided,
                           float w, const float* w_dev, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sched,
                           const mi355_multistep_schedule* msched, const float* noise, int64_t n_noise_draws, int batch, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  const std::string f = std::string(o.who) + ": ";
  const mi355_ddpm_variance* const var = o.var;
  const mi355_x0_shaping* const shaping = o.shaping;
  MI355_REQUIRE(tb && opt, -1, f + "tables or opt is null");
  MI355_REQUIRE(!(sched && msched), -1, f + "both sched and msched given (a run follows one schedule)");
  const DdpmGuidance g{labels, null_label, w, w_dev};
  DdpmCall c = ddpm_call(o.who, batch, guided ? &g : nullptr);
  const int K = tb->Ns;
  if (o.pred) {   // these refusals need no handle
    MI355_REQUIRE(o.pred->kind >= PRED_EPS && o.pred->kind <= PRED_V, -1, f + "pred->kind must be 0 (eps), 1 (x0) or 2 (v)");
    if (o.pred->kind == PRED_V)
      MI355_REQUIRE((tb->sqrt_alphas_cumprod && tb->sqrt_one_minus_alphas_cumprod) || K <= 0, -1,
                    f + "pred->kind 2 (v) needs tables->sqrt_alphas_cumprod and tables->sqrt_one_minus_alphas_cumprod");
    c.ls.pred = o.pred->kind;
  }
  if (var) {
    MI355_REQUIRE(var->learned == 0 || var->learned == 1, -1, f + "var->learned must be 0 (the tables' fixed variance) or 1 (the learned range)");
    MI355_REQUIRE(!var->learned || var->max_log || K <= 0, -1, f + "var->learned needs var->max_log (log(betas[k]) of the chain)");
    for (int k = 0; var->learned && k < K; ++k) MI355_REQUIRE(std::isfinite(var->max_log[k]), -1, f + "var->max_log must be finite");
    for (int k = 0; var->times && k < K; ++k) MI355_REQUIRE(std::isfinite(var->times[k]), -1, f + "var->times must be finite");
  }
  if (int rc = check_x0_shaping(o.who, shaping, guided)) return rc;
  const bool shaped = shaping && (shaping->quantile > 0.f || shaping->rescale_phi > 0.f);
  MI355_REQUIRE(!(shaped && var && var->learned), -1, f + "var->learned together with shaping: per-image shaping rows are not built for the learned-variance step");
  const LoopSched keep = c.ls;   // check_schedule starts its LoopSched afresh
  mi355_ddpm_schedule sd;
  if (msched) {
    MI355_REQUIRE(!noise, -1, f + "noise given with msched (the multistep solver is deterministic and draws none)");
    if (int rc = check_multistep(c.who, tb, opt, msched, c.spec.guided, sd, c.ls)) return rc;
    c.th = sched_times(K, &sd);
  } else if (sched) {
    if (int rc = check_schedule(c.who, tb, opt, sched, c.spec.guided, c.ls)) return rc;
    c.th = sched_times(K, sched);
  } else {
    c.th = ddpm_times(K);
  }
  c.ls.pred = keep.pred;
  MI355_REQUIRE(net && x && workspace && batch > 0, -1, f + "bad argument (net, x, workspace, batch)");
  if (var && var->times) c.th.assign(var->times, var->times + (K > 0 ? K : 0));
  if (var && var->learned && K > 0) c.ls.lv_max_log = var->max_log;
  c.spec.hist = msched != nullptr; c.spec.rows = o.rows; c.spec.lv = o.lv; c.count_step = true;
  if (shaped) c.ls.shaping = shaping;   // off: the unshaped loop, bit for bit
  return ddpm_run(c, net, x, channels, cond, tb, opt, noise, n_noise_draws, workspace, workspace_bytes, stream);
}

int mi355_ddpm_shaped_sample(mi355_unet* net, float* x, int channels, const float* cond, const int32_t* labels, int null_label, int guided, float w,
                             const float* w_dev, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sched,
                             const mi355_multistep_schedule* msched, const mi355_x0_shaping* shaping, const float* noise, int64_t n_noise_draws,
                             int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  const OverLoops o{"ddpm_shaped_sample", true, false, nullptr, shaping, nullptr};
  return ddpm_over_loops(o, net, x, channels, cond, labels, null_label, guided, w, w_dev, tb, opt, sched, msched, noise, n_noise_draws, batch, workspace,
                         workspace_bytes, stream);
}

// Learned-variance nets (improved DDPM's learned range) and caller-given evaluation times: one entry point over the six loops above.  var null, or
// neither learned nor times: the loop chosen runs as its own entry point does, bit for bit.
int64_t mi355_ddpm_lv_workspace_bytes(const mi355_unet* net, int batch, int guided, int multistep) {
  if (!net || batch <= 0) { mi355_set_error("ddpm_lv_workspace_bytes: bad argument"); return -1; }
  LayoutSpec sp = plain_spec(batch, guided != 0);
  sp.hist = multistep != 0; sp.lv = true;
  return layout_bytes(net, sp);
}

int mi355_ddpm_lv_sample(mi355_unet* net, float* x, int channels, const float* cond, const int32_t* labels, int null_label, int guided, float w,
                         const float* w_dev, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sched,
                         const mi355_multistep_schedule* msched, const mi355_ddpm_variance* var, const float* noise, int64_t n_noise_draws, int batch,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  const OverLoops o{"ddpm_lv_sample", false, true, var, nullptr, nullptr};
  return ddpm_over_loops(o, net, x, channels, cond, labels, null_label, guided, w, w_dev, tb, opt, sched, msched, noise, n_noise_draws, batch, workspace,
                         workspace_bytes, stream);
}

// x0- and v-prediction nets (mi355_ddpm_prediction): the entry point above with the shaping rows and the prediction kind beside the variance.  pred null
// or kind 0: the loop the other arguments choose, bit for bit.
int64_t mi355_ddpm_pred_workspace_bytes(const mi355_unet* net, int batch, int guided, int multistep) {
  if (!net || batch <= 0) { mi355_set_error("ddpm_pred_workspace_bytes: bad argument"); return -1; }
  LayoutSpec sp = plain_spec(batch, guided != 0);
  sp.hist = multistep != 0; sp.rows = true; sp.lv = true;
  return layout_bytes(net, sp);
}

int mi355_ddpm_pred_sample(mi355_unet* net, float* x, int channels, const float* cond, const int32_t* labels, int null_label, int guided, float w,
                           const float* w_dev, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sched,
                           const mi355_multistep_schedule* msched, const mi355_ddpm_variance* var, const mi355_x0_shaping* shaping,
                           const mi355_ddpm_prediction* pred, const float* noise, int64_t n_noise_draws, int batch, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  const OverLoops o{"ddpm_pred_sample", true, true, var, shaping, pred};
  return ddpm_over_loops(o, net, x, channels, cond, labels, null_label, guided, w, w_dev, tb, opt, sched, msched, noise, n_noise_draws, batch, workspace,
                         workspace_bytes, stream);
}

// Null-space (DDNM) restoration: the scheduled loop with the null-space predictor (LoopSched::ns_op).  Every refusal before any launch.
int64_t mi355_ddpm_nullspace_workspace_bytes(const mi355_unet* net, int batch) {
  if (!net || batch <= 0) { mi355_set_error("ddpm_nullspace_workspace_bytes: bad argument"); return -1; }
  return layout_bytes(net, plain_spec(batch));
}

int mi355_ddpm_nullspace_sample(mi355_unet* net, float* x, int channels, const float* y, const mi355_nullspace_op* op, const int32_t* labels,
                                const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const mi355_ddpm_schedule* sched,
                                const mi355_nullspace_schedule* ns, const mi355_ddpm_prediction* pred, const float* noise, int64_t n_noise_draws,
                                int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const who = "ddpm_nullspace_sample";
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(tb && opt, -1, f + "tables or opt is null");
  MI355_REQUIRE(y, -1, f + "y is null");
  MI355_REQUIRE(op, -1, f + "op is null");
  MI355_REQUIRE(ns, -1, f + "ns is null");
  MI355_REQUIRE(opt->mode == MI355_DDPM_PRIOR || opt->mode == MI355_DDIM, -1,
                f + "opt->mode must be MI355_DDPM_PRIOR (form 0, the ancestral step) or MI355_DDIM (form 1)");
  MI355_REQUIRE(opt->n_corrector == 0, -1, f + "opt->n_corrector must be 0 (no corrector is built behind the null-space step)");
  const int K = tb->Ns;
  const bool form1 = opt->mode == MI355_DDIM;
  MI355_REQUIRE(form1 || ns->sigma || K <= 0, -1, f + "ns->sigma is null (form 0 takes the noise std of every step from it)");
  MI355_REQUIRE(!form1 || !ns->sigma, -1, f + "ns->sigma given in form 1 (MI355_DDIM takes its sigma from sched->ddim_sigma)");
  MI355_REQUIRE(ns->lam || K <= 0, -1, f + "ns->lam is null");
  for (int k = 0; k < K; ++k) {
    MI355_REQUIRE(ns->lam[k] >= 0.f && ns->lam[k] <= 3.0e38f, -1, f + "ns->lam must be finite and >= 0");
    MI355_REQUIRE(ns->lam[k] <= 1.f, -1, f + "ns->lam must be <= 1");
    if (ns->sigma) MI355_REQUIRE(ns->sigma[k] >= 0.f && ns->sigma[k] <= 3.0e38f, -1, f + "ns->sigma must be finite and >= 0");
  }
  DdpmCall c = ddpm_call(who, batch, nullptr);
  if (pred) {
    MI355_REQUIRE(pred->kind >= PRED_EPS && pred->kind <= PRED_V, -1, f + "pred->kind must be 0 (eps), 1 (x0) or 2 (v)");
    if (pred->kind == PRED_V)
      MI355_REQUIRE((tb->sqrt_alphas_cumprod && tb->sqrt_one_minus_alphas_cumprod) || K <= 0, -1,
                    f + "pred->kind 2 (v) needs tables->sqrt_alphas_cumprod and tables->sqrt_one_minus_alphas_cumprod");
  }
  if (sched) {
    if (int rc = check_schedule(who, tb, opt, sched, false, c.ls)) return rc;   // starts c.ls afresh
    c.th = sched_times(K, sched);
  } else {
    c.th = ddpm_times(K);
  }
  MI355_REQUIRE(net && x && workspace && batch > 0, -1, f + "bad argument (net, x, workspace, batch)");
  MI355_REQUIRE(net->cfg.in_channels == channels, -2,
                f + "net: an unconditional net is needed (in_channels == channels; a 2C-input amortized net sees a condition this sampler does not give)");
  MI355_REQUIRE(net->cfg.out_channels == channels || net->cfg.out_channels == 2 * channels, -2, f + "net: out_channels must be channels or 2 * channels");
  const bool wide = net->cfg.out_channels == 2 * channels;
  MI355_REQUIRE(!wide || form1, -2,
                f + "net: a 2C-output (learned-variance) net is read in form 1 (MI355_DDIM) alone: its variance and DDNM+'s are not reconciled");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, f + "labels: class labels given to a net built without num_classes");
  if (int rc = check_nullspace_op(who, op, net->cfg.image_size, net->cfg.image_size)) return rc;
  if (pred) c.ls.pred = pred->kind;
  c.ls.ns_op = op; c.ls.ns_y = y; c.ls.ns_lam = ns->lam; c.ls.ns_sigma = ns->sigma; c.ls.wide_out = wide;
  c.labels = labels; c.count_step = true;
  return ddpm_run(c, net, x, channels, nullptr, tb, opt, noise, n_noise_draws, workspace, workspace_bytes, stream);
}

// The variational bound of a DDPM net on data x0 (the formulas: include/mi355_sampler.h): steps K-1 .. 0, each the noising launch into the workspace's
// resident state, the evaluation, the terms launch (vlb.hip); then the prior term and the totals.  x0 is read by every step and never written.
int64_t mi355_ddpm_vlb_workspace_bytes(const mi355_unet* net, int batch) {
  if (!net || batch <= 0) { mi355_set_error("ddpm_vlb_workspace_bytes: bad argument"); return -1; }
  return layout_bytes(net, plain_spec(batch));
}

// the body of mi355_ddpm_vlb and mi355_ddpm_vlb_pred; pred: a checked PRED_* kind
static int ddpm_vlb_run(int pred, mi355_unet* net, const float* x0, int channels, const float* cond, const int32_t* labels, const mi355_ddpm_tables* tb,
                        const mi355_vlb_options* opt, const float* noise, int64_t n_noise_draws, float* out_terms, float* summary, int batch,
                        void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(tb, -1, "ddpm_vlb: tables is null");
  MI355_REQUIRE(opt, -1, "ddpm_vlb: opt is null");
  const int K = tb->Ns;
  MI355_REQUIRE(K >= 2, -1, "ddpm_vlb: tables->Ns must be >= 2 (the bound has a decoder step and at least one KL step)");
  MI355_REQUIRE(opt->learned == 0 || opt->learned == 1, -1, "ddpm_vlb: opt->learned must be 0 (the fixed model_log) or 1 (the learned range)");
  MI355_REQUIRE(opt->cdf == 0 || opt->cdf == 1, -1, "ddpm_vlb: opt->cdf must be 0 (exact, erfc) or 1 (the tanh approximation)");
  MI355_REQUIRE(opt->clip_denoised == 0 || opt->clip_denoised == 1, -1, "ddpm_vlb: opt->clip_denoised must be 0 or 1");
  const bool learned = opt->learned != 0;
  // every table the mode reads: present and finite (DDPM(Ns <= 20) has non-finite chain tables and is refused here)
  const struct { const float* p; const char* name; bool read; } tabs[] = {
      {opt->true_log, "opt->true_log", true}, {opt->model_log, "opt->model_log", !learned}, {opt->min_log, "opt->min_log", learned},
      {opt->max_log, "opt->max_log", learned}, {tb->sqrt_recip_alphas_cumprod, "tables->sqrt_recip_alphas_cumprod", true},
      {tb->sqrt_recipm1_alphas_cumprod, "tables->sqrt_recipm1_alphas_cumprod", true}, {tb->posterior_mean_coef1, "tables->posterior_mean_coef1", true},
      {tb->posterior_mean_coef2, "tables->posterior_mean_coef2", true}, {tb->sqrt_alphas_cumprod, "tables->sqrt_alphas_cumprod", true},
      {tb->sqrt_one_minus_alphas_cumprod, "tables->sqrt_one_minus_alphas_cumprod", true}};
  for (const auto& t : tabs) {
    if (!t.read) continue;
    MI355_REQUIRE(t.p, -1, std::string("ddpm_vlb: ") + t.name + " is null");
    for (int k = 0; k < K; ++k) MI355_REQUIRE(std::isfinite(t.p[k]), -1, std::string("ddpm_vlb: ") + t.name + " must be finite");
  }
  MI355_REQUIRE(tb->sqrt_one_minus_alphas_cumprod[K - 1] > 0.f, -1, "ddpm_vlb: tables->sqrt_one_minus_alphas_cumprod[K-1] must be > 0 (the prior term takes its log)");
  for (int k = 0; opt->times && k < K; ++k) MI355_REQUIRE(std::isfinite(opt->times[k]), -1, "ddpm_vlb: opt->times must be finite");
  MI355_REQUIRE(net, -1, "ddpm_vlb: net is null");
  MI355_REQUIRE(x0, -1, "ddpm_vlb: x0 is null");
  MI355_REQUIRE(out_terms, -1, "ddpm_vlb: out_terms is null");
  MI355_REQUIRE(summary, -1, "ddpm_vlb: summary is null");
  MI355_REQUIRE(workspace, -1, "ddpm_vlb: workspace is null");
  MI355_REQUIRE(batch > 0 && channels > 0, -1, "ddpm_vlb: batch and channels must be > 0");
  MI355_REQUIRE(!learned || net->cfg.out_channels == 2 * channels, -2,
                "ddpm_vlb: opt->learned needs a net whose out_channels == 2 * channels (eps and the variance channels)");
  MI355_REQUIRE(learned || net->cfg.out_channels == channels, -2,
                "ddpm_vlb: a fixed variance (opt->learned == 0) needs a net whose out_channels == channels");
  const bool amortized = net->cfg.in_channels == 2 * channels;
  MI355_REQUIRE(amortized || net->cfg.in_channels == channels, -2, "ddpm_vlb: network in_channels must be channels or 2 * channels");
  MI355_REQUIRE(!cond || amortized, -2, "ddpm_vlb: cond given to a net that takes no condition (in_channels == channels)");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "ddpm_vlb: labels given to a net built without num_classes");
  MI355_REQUIRE(!noise || n_noise_draws >= K, -2, "ddpm_vlb: injected noise exhausted (noise holds fewer than tables->Ns draws)");
  Layout l;
  if (int rc = carve(net, plain_spec(batch), workspace, workspace_bytes, l, "ddpm_vlb")) return rc;
  const Scratch& sc = l.sc;
  hipStream_t s = S(stream);
  const int64_t hw = (int64_t)net->cfg.image_size * net->cfg.image_size;
  const int64_t per = (int64_t)channels * hw, n = (int64_t)batch * per, n_al = (n + 3) / 4 * 4;
  const std::vector<float> th = opt->times ? std::vector<float>(opt->times, opt->times + K) : ddpm_times(K);
  EvalEmb emb;   // row k (block of num_classes rows with labels) = step k
  if (int rc = emb.init(net, sc, th.data(), K, labels != nullptr, true, s)) return rc;
  if (amortized && !cond) { if (int rc = fill_launch(sc.none, opt->none_value, n, s)) return rc; }
  const float* const condp = amortized ? (cond ? cond : sc.none) : nullptr;
  float* const xk = sc.xstate;   // [batch, out_channels, H, W] floats: room for the state's channels
  UnetRun run = uniform_t_run();
  run.labels = labels;
  VlbStep st;
  st.learned = opt->learned; st.cdf = opt->cdf; st.clip = opt->clip_denoised; st.pred = pred;
  for (int k = K - 1; k >= 0; --k) {
    const int64_t draw = K - 1 - k;
    const float* const z = noise ? noise + (size_t)draw * n : nullptr;
    const int philox = noise ? 0 : 1;
    const uint64_t off = noise ? 0 : (uint64_t)draw * (uint64_t)n_al;
    int rc;
    if ((rc = q_sample_launch(xk, x0, z, tb->sqrt_alphas_cumprod[k], tb->sqrt_one_minus_alphas_cumprod[k], philox, opt->seed, off, n, s))) return rc;
    if ((rc = emb.select(run, (size_t)k, batch, s))) return rc;
    if ((rc = unet_forward(net, xk, channels, condp, channels, sc.t, sc.v, batch, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
    st.c_recip = tb->sqrt_recip_alphas_cumprod[k]; st.c_recipm1 = tb->sqrt_recipm1_alphas_cumprod[k];
    st.sa = tb->sqrt_alphas_cumprod[k]; st.sb = tb->sqrt_one_minus_alphas_cumprod[k];
    st.coef1 = tb->posterior_mean_coef1[k]; st.coef2 = tb->posterior_mean_coef2[k];
    st.true_log = opt->true_log[k];
    if (learned) { st.min_log = opt->min_log[k]; st.max_log = opt->max_log[k]; }
    else st.model_log = opt->model_log[k];
    st.k_is_zero = k == 0;
    if ((rc = vlb_terms_launch(x0, xk, sc.v, (int64_t)net->cfg.out_channels * hw, z, philox, opt->seed, off, st, out_terms + 3 * (size_t)k, 3 * (int64_t)K,
                               batch, per, s))) return rc;
  }
  if (int rc = vlb_prior_launch(x0, tb->sqrt_alphas_cumprod[K - 1], tb->sqrt_one_minus_alphas_cumprod[K - 1], out_terms, 3 * (int64_t)K, K, summary, batch,
                                per, s)) return rc;
  net->last_launches += 2;   // the last evaluation with its noising and terms launches
  return 0;
}

int mi355_ddpm_vlb(mi355_unet* net, const float* x0, int channels, const float* cond, const int32_t* labels, const mi355_ddpm_tables* tb,
                   const mi355_vlb_options* opt, const float* noise, int64_t n_noise_draws, float* out_terms, float* summary, int batch, void* workspace,
                   int64_t workspace_bytes, void* stream) {
  return ddpm_vlb_run(PRED_EPS, net, x0, channels, cond, labels, tb, opt, noise, n_noise_draws, out_terms, summary, batch, workspace, workspace_bytes, stream);
}

int mi355_ddpm_vlb_pred(mi355_unet* net, const float* x0, int channels, const float* cond, const int32_t* labels, const mi355_ddpm_tables* tb,
                        const mi355_vlb_options* opt, const mi355_ddpm_prediction* pred, const float* noise, int64_t n_noise_draws, float* out_terms,
                        float* summary, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(!pred || (pred->kind >= PRED_EPS && pred->kind <= PRED_V), -1, "ddpm_vlb_pred: pred->kind must be 0 (eps), 1 (x0) or 2 (v)");
  return ddpm_vlb_run(pred ? pred->kind : PRED_EPS, net, x0, channels, cond, labels, tb, opt, noise, n_noise_draws, out_terms, summary, batch, workspace,
                      workspace_bytes, stream);
}

// Adams-Bashforth CFM samplers: the loop of mi355_cfm_rk_sample / mi355_cfm_cfg_sample with the tableau as the start method (cfm_rk_loop, AbPlan).
namespace {
int check_ab(const char* who, int order, const float* w_host, int n_t, int stages, const float* a_host, const float* b_host, const float* c_host) {
  const std::string f = std::string(who) + ": ";
  MI355_REQUIRE(order >= 2 && order <= 4, -1, f + "order must be 2, 3 or 4");
  MI355_REQUIRE(w_host, -1, f + "w_host is null");
  if (int rc = check_tableau(who, stages, a_host, b_host, c_host)) return rc;
  MI355_REQUIRE(c_host[0] == 0.f, -1, f + "c_host[0] must be 0: the start method's first stage is the history sample v(t_k, x_k)");
  for (int k = order - 1; k + 1 < n_t; ++k) {
    bool any = false;
    for (int j = 0; j < order; ++j) {
      MI355_REQUIRE(std::isfinite(w_host[(size_t)k * order + j]), -1, f + "w_host must be finite");
      any = any || w_host[(size_t)k * order + j] != 0.f;
    }
    MI355_REQUIRE(any, -1, f + "w_host has an all-zero row at a multistep step");
  }
  return 0;
}
}  // namespace

int64_t mi355_cfm_ab_workspace_bytes(const mi355_unet* net, int batch, int order, int start_stages, int guided) {
  if (!net || batch <= 0 || order < 2 || order > 4 || start_stages < 1 || start_stages > 4) {
    mi355_set_error("cfm_ab_workspace_bytes: bad argument (2 <= order <= 4, 1 <= start_stages <= 4)");
    return -1;
  }
  return layout_bytes(net, plain_spec(batch, guided != 0, order + start_stages - 1));
}

// Adams-Bashforth entry points: check_ab needs no handle and runs before the handle checks.
int mi355_cfm_ab_sample(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, const int32_t* labels, const float* t_span_host,
                        int n_t, int order, const float* w_host, int start_stages, const float* a_host, const float* b_host, const float* c_host,
                        float* traj, uint8_t* u8_out, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(t_span_host && n_t >= 1, -1, "cfm_ab_sample: t_span_host is null or empty");
  if (int rc = check_ab("cfm_ab_sample", order, w_host, n_t, start_stages, a_host, b_host, c_host)) return rc;
  MI355_REQUIRE(net && x && batch > 0, -1, "cfm_ab_sample: bad argument (net, x, batch)");
  const AbPlan ab{order, w_host};
  CfmCall c{"cfm_ab_sample", start_stages, a_host, b_host, c_host};
  c.ab = &ab;
  return cfm_fixed_run(c, net, x, x_channels, cond, cond_channels, labels, t_span_host, n_t, traj, u8_out, batch, workspace, workspace_bytes, stream);
}

int mi355_cfm_ab_cfg_sample(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, float none_value, const int32_t* labels,
                            int null_label, float w, const float* w_dev, const float* t_span_host, int n_t, int order, const float* w_host,
                            int start_stages, const float* a_host, const float* b_host, const float* c_host, float* traj, uint8_t* u8_out, int batch,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(t_span_host && n_t >= 1, -1, "cfm_ab_cfg_sample: t_span_host is null or empty");
  if (int rc = check_ab("cfm_ab_cfg_sample", order, w_host, n_t, start_stages, a_host, b_host, c_host)) return rc;
  MI355_REQUIRE(net && x && batch > 0, -1, "cfm_ab_cfg_sample: bad argument (net, x, batch)");
  const CfmGuidance g{none_value, null_label, w, w_dev};
  const AbPlan ab{order, w_host};
  CfmCall c{"cfm_ab_cfg_sample", start_stages, a_host, b_host, c_host};
  c.guided = &g; c.ab = &ab;
  return cfm_fixed_run(c, net, x, x_channels, cond, cond_channels, labels, t_span_host, n_t, traj, u8_out, batch, workspace, workspace_bytes, stream);
}

// Training-free in-painting / super-resolution of an unconditional flow: replacement along the straight path and / or reconstruction guidance
// through the data estimate x1_hat = x + (1 - t) v, one Euler step per interval (include/mi355_sampler.h).  A guided step is forward -> seed ->
// unet_backward -> ONE rk_stage launch over (v, g_x, vjp); an unguided one the stage launch over v alone.
int64_t mi355_cfm_recon_workspace_bytes(const mi355_unet* net, int batch, int h_low, int w_low) {
  if (!net || batch <= 0 || h_low < 0 || w_low < 0) { mi355_set_error("cfm_recon_workspace_bytes: bad argument"); return -1; }
  const ReconDims rd{h_low, w_low};
  LayoutSpec sp = plain_spec(batch);
  sp.recon = &rd;
  return layout_bytes(net, sp);
}

int mi355_cfm_recon_sample(mi355_unet* net, float* x, int channels, const int32_t* labels, const float* t_span_host, int n_t, const float* y, int mode,
                           float pad_value, int h_low, int w_low, const float* scales_host, int replace, int final_paste, const float* z, uint64_t seed,
                           float* traj, uint8_t* u8_out, float* loss_out, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && t_span_host && batch > 0, -1, "cfm_recon_sample: bad argument");
  MI355_REQUIRE(n_t >= 1, -1, "cfm_recon_sample: the time span needs at least one time (n_t >= 1)");
  MI355_REQUIRE(mode >= 0 && mode <= 2, -1, "cfm_recon_sample: mode must be 0 (painting), 1 (hyper-resolution) or 2 (low resolution)");
  MI355_REQUIRE(replace >= 0 && replace <= 2, -1, "cfm_recon_sample: replace must be 0 (off), 1 (coupled) or 2 (fresh)");
  MI355_REQUIRE(replace == 0 || mode == 0, -1, "cfm_recon_sample: replacement pastes the known pixels of a painting condition (mode 0)");
  MI355_REQUIRE(final_paste == 0 || replace != 0, -1, "cfm_recon_sample: final_paste is the replacement's last paste (replace != 0)");
  MI355_REQUIRE(net->cfg.in_channels == net->cfg.out_channels, -2,
                "cfm_recon_sample: needs an unconditional net, in_channels == out_channels (amortized nets are not for this sampler)");
  MI355_REQUIRE(channels == net->cfg.out_channels, -2, "cfm_recon_sample: the vector field must have the state's channel count");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "cfm_recon_sample: class labels given to a net built without num_classes");
  bool any_scale = false;
  for (int k = 0; scales_host && k + 1 < n_t; ++k) any_scale = any_scale || scales_host[k] != 0.f;
  MI355_REQUIRE(y || (replace == 0 && !any_scale), -1, "cfm_recon_sample: replacement and guidance need the measurement y");
  MI355_REQUIRE(!any_scale || net->cfg.differentiable, -4, "unet_vjp: the handle was not created with cfg.differentiable = 1");
  MI355_REQUIRE(!loss_out || mode == 2, -1, "cfm_recon_sample: the per-step loss is the low-resolution seed's (mode 2)");
  const int H = net->cfg.image_size, W = net->cfg.image_size;
  if (mode == 2) {
    MI355_REQUIRE(h_low > 0 && w_low > 0, -1, "cfm_recon_sample: mode 2 needs the low resolution (h_low, w_low)");
    MI355_REQUIRE(H % h_low == 0 && W % w_low == 0, -4, "cfm_recon_sample: the low resolution must divide the state's (integer factors only)");
  }
  const ReconDims rd{mode == 2 ? h_low : 0, mode == 2 ? w_low : 0};
  LayoutSpec sp = plain_spec(batch);
  sp.recon = &rd;
  Layout l;
  if (int rc = carve(net, sp, workspace, workspace_bytes, l)) return rc;
  const Scratch& sc = l.sc;
  const ReconTail& rt = l.rec;
  hipStream_t s = S(stream);
  const int64_t per = (int64_t)channels * H * W, n = (int64_t)batch * per, n_al = (n + 3) / 4 * 4;
  const int n_steps = n_t - 1;
  EvalEmb emb;   // t_span_host is the caller's array: no wait
  if (int rc = emb.init(net, sc, t_span_host, n_steps, labels != nullptr, false, s)) return rc;
  if (replace == 1) MI355_CHECK_HIP(hipMemcpyAsync(rt.x_init, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  if (loss_out && n_steps > 0)   // rows of unguided steps: NaN (no loss was formed)
    if (int rc = fill_launch(loss_out, __builtin_nanf(""), (int64_t)n_steps * batch, s)) return rc;
  // x <- where(y == pad, x, t y + (1 - t) z_k): the known pixels on the straight path from the noise z_k to the measurement
  auto paste = [&](int k) -> int {
    const float t = t_span_host[k], omt = 1.0f - t;
    const float* zk = replace == 1 ? rt.x_init : (z ? z + (size_t)k * n : nullptr);
    return replace_mask_launch(x, y, zk, pad_value, 1, t, omt, zk ? 0 : 1, seed, zk ? 0 : (uint64_t)k * (uint64_t)n_al, n, s);
  };
  int64_t vjp_ops = 1;   // the adjoint ops unet_backward walks (each one or more launches) and its unpack: what a guided step adds to the count
  for (const PlanOp& op : net->ops) vjp_ops += op.kind != OP_GN;
  UnetRun run = uniform_t_run();   // no euler_x: the last conv stores v
  run.labels = labels;
  int64_t step_launches = 0;
  int rc = 0;
  for (int k = 0; k < n_steps; ++k) {
    const float t = t_span_host[k], dt = t_span_host[k + 1] - t, omt = 1.0f - t;
    step_launches = 0;
    if (replace) { if ((rc = paste(k))) return rc; ++step_launches; }
    if ((rc = emb.select(run, (size_t)k, batch, s, &step_launches))) return rc;
    if ((rc = unet_forward(net, x, channels, nullptr, 0, sc.t, sc.v, batch, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
    step_launches += net->last_launches;
    const float sk = scales_host ? scales_host[k] : 0.f;
    const float* kp[4] = {sc.v, rt.g_x, rt.vjp, nullptr};
    float cf[4] = {dt, 0.f, 0.f, 0.f};
    int nk = 1;
    if (sk != 0.f) {
      // x1_hat = 1 * x - (-(1 - t)) * v: the seed kernels' pre = c_recip x - c_recipm1 eps with c_recip = 1, c_recipm1 = -(1 - t)
      if (mode == 2) {
        float* lk = loss_out ? loss_out + (size_t)k * batch : nullptr;
        rc = lowres_seed_launch(x, sc.v, y, 1.f, -omt, batch, channels, H, W, h_low, w_low, rt.resid, rt.g_eps, rt.g_x, lk, s);
        step_launches += lk ? 3 : 2;
      } else {
        rc = guidance_seed_launch(x, sc.v, y, 1.f, -omt, mode, pad_value, per, rt.g_eps, rt.g_x, n, s);
        ++step_launches;
      }
      if (rc) return rc;
      if ((rc = unet_backward(net, rt.g_eps, rt.vjp, channels, batch, sc.unet_ws, sc.unet_bytes, s))) return rc;
      step_launches += vjp_ops;
      const float c = dt * sk;   // rounded to fp32 here: x <- x + dt v - c g_x - c vjp
      cf[1] = -c; cf[2] = -c; nk = 3;
    }
    const bool last = k + 1 == n_steps;
    if ((rc = rk_stage_launch(x, x, kp, cf, nk, n, traj ? traj + (size_t)(k + 1) * n : nullptr, last && !final_paste ? u8_out : nullptr, s))) return rc;
    ++step_launches;
  }
  if (final_paste) {   // at t = 1 this is 1 * y + 0 * z: the known pixels are the measurement itself
    if ((rc = paste(n_t - 1))) return rc;
    if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj + (size_t)n_steps * n, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  }
  if (u8_out && (final_paste || n_steps == 0) && (rc = quantize_u8_launch(x, u8_out, n, s))) return rc;
  if (n_steps > 0) net->last_launches = step_launches;   // mi355_unet_get_stats: the launches of the last step
  return 0;
}

// SF2M (torchcfm notebooks' torchsde.sdeint of drift = model + score_model, g = sigma): per step two forwards, each net on its own workspace
// (its own embedding table: label_emb differs between the nets), then the Euler-Maruyama launch, which also writes the step's output time.
int mi355_sf2m_euler_sample(mi355_unet* drift, mi355_unet* score, float* x, int channels, const int32_t* labels, const float* t_grid_host,
                            int n_steps, float sigma, int reverse, const float* dW, uint64_t seed, const int32_t* out_step_host,
                            const float* out_w_host, int n_out, float* traj, int batch, void* drift_workspace, int64_t drift_workspace_bytes,
                            void* score_workspace, int64_t score_workspace_bytes, void* stream) {
  MI355_REQUIRE(drift && score && x && t_grid_host && batch > 0, -1, "sf2m_euler_sample: bad argument");
  MI355_REQUIRE(n_steps >= 1, -1, "sf2m_euler_sample: the step grid needs at least one step (n_steps >= 1)");
  MI355_REQUIRE(drift_workspace != score_workspace, -1, "sf2m_euler_sample: the two nets need separate workspaces");
  const mi355_unet_config &cd = drift->cfg, &cs = score->cfg;
  MI355_REQUIRE(cd.in_channels == cs.in_channels && cd.out_channels == cs.out_channels && cd.image_size == cs.image_size, -2,
                "sf2m_euler_sample: the drift and score nets differ in in_channels, out_channels or image_size");
  MI355_REQUIRE(cd.in_channels == channels && cd.out_channels == channels, -2,
                "sf2m_euler_sample: both nets must map the state's channel count to itself (in_channels == out_channels == channels)");
  MI355_REQUIRE(!labels || (drift->num_classes > 0 && score->num_classes > 0), -1,
                "sf2m_euler_sample: class labels given to a net built without num_classes (both nets must be class-conditional)");
  MI355_REQUIRE(!labels || drift->num_classes == score->num_classes, -1, "sf2m_euler_sample: the two class-conditional nets differ in num_classes");
  MI355_REQUIRE(n_out == 0 || (traj && out_step_host && out_w_host), -1, "sf2m_euler_sample: outputs need traj, out_step and out_w");
  for (int j = 0; j < n_out; ++j)
    MI355_REQUIRE(out_step_host[j] >= 0 && out_step_host[j] < n_steps && out_w_host[j] >= 0.f && out_w_host[j] <= 1.f, -1,
                  "sf2m_euler_sample: an output's step must be in [0, n_steps) and its weight in [0, 1]");
  Layout ld, ls;
  if (int rc = carve(drift, plain_spec(batch), drift_workspace, drift_workspace_bytes, ld)) return rc;
  if (int rc = carve(score, plain_spec(batch), score_workspace, score_workspace_bytes, ls)) return rc;
  const Scratch &sd = ld.sc, &ss = ls.sc;
  hipStream_t s = S(stream);
  const int64_t n = (int64_t)batch * channels * cd.image_size * cd.image_size;
  const int64_t n_al = (n + 3) / 4 * 4;
  // the times the nets see: t_k, or 1 - t_k rounded in fp32 (the notebook's reverse SDE evaluates at `1 - t` of the fp32 tensor)
  std::vector<float> te((size_t)n_steps);
  for (int k = 0; k < n_steps; ++k) te[k] = reverse ? 1.0f - t_grid_host[k] : t_grid_host[k];
  EvalEmb ed, es;
  if (int rc = ed.init(drift, sd, te.data(), n_steps, labels != nullptr, false, s)) return rc;
  if (int rc = es.init(score, ss, te.data(), n_steps, labels != nullptr, false, s)) return rc;
  if (ed.table() || es.table()) MI355_CHECK_HIP(hipStreamSynchronize(s));   // `te` is a temporary host buffer: ONE wait for both copies
  UnetRun rd = uniform_t_run(), rs = uniform_t_run();
  rd.labels = rs.labels = labels;
  const float ca = reverse ? -1.f : 1.f;
  int rc = 0;
  for (int k = 0; k < n_steps && rc == 0; ++k) {
    const float dt = t_grid_host[k + 1] - t_grid_host[k];
    if ((rc = ed.select(rd, (size_t)k, batch, s))) break;
    if ((rc = es.select(rs, (size_t)k, batch, s))) break;
    if ((rc = unet_forward(drift, x, channels, nullptr, 0, sd.t, sd.v, batch, sd.unet_ws, sd.unet_bytes, s, rd))) break;
    if ((rc = unet_forward(score, x, channels, nullptr, 0, ss.t, ss.v, batch, ss.unet_ws, ss.unet_bytes, s, rs))) break;
    const float* dw = dW ? dW + (size_t)k * n : nullptr;
    const uint64_t off = dW ? 0 : (uint64_t)k * (uint64_t)n_al;
    // outputs of this step: w == 0 is x_k itself (copied before the update); the first other one rides in the step launch; further ones
    // (several output times inside one step) re-run the same deterministic update on a copy of x_k held in the drift net's spare scratch
    float* fused = nullptr; float fused_w = 0.f;
    for (int j = 0; j < n_out && rc == 0; ++j) {
      if (out_step_host[j] != k) continue;
      float* oj = traj + (size_t)j * n;
      if (out_w_host[j] == 0.f) { MI355_CHECK_HIP(hipMemcpyAsync(oj, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s)); continue; }
      if (!fused) { fused = oj; fused_w = out_w_host[j]; continue; }
      MI355_REQUIRE(channels <= 32, -4, "sf2m_euler_sample: several output times inside one step need channels <= 32");
      MI355_CHECK_HIP(hipMemcpyAsync(sd.none, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
      rc = sde_euler_step_launch(sd.none, sd.v, ss.v, ca, 1.f, dt, nullptr, sigma, dw, !dW, seed, off, oj, out_w_host[j], n, s);
    }
    if (rc) break;
    rc = sde_euler_step_launch(x, sd.v, ss.v, ca, 1.f, dt, nullptr, sigma, dw, !dW, seed, off, fused, fused_w, n, s);
  }
  return rc;
}

// ---- tiled sampling: the entry points (TiledEval; include/mi355_sampler.h) -------------------------------------------------------------------
int mi355_tile_count(int image_size, const mi355_tile_plan* plan, int32_t out[3]) {
  MI355_REQUIRE(out, -1, "tile_count: out is null");
  TileGeom g;
  if (int rc = tile_geom(image_size, plan, &g, "tile_count")) return rc;
  out[0] = g.ny; out[1] = g.nx; out[2] = g.nW;
  return 0;
}

int mi355_tile_origins(int image_size, const mi355_tile_plan* plan, int32_t* oy, int32_t* ox) {
  MI355_REQUIRE(oy && ox, -1, "tile_origins: oy or ox is null");
  TileGeom g;
  if (int rc = tile_geom(image_size, plan, &g, "tile_origins")) return rc;
  for (int i = 0; i < g.ny; ++i) oy[i] = tile_origin(i, g.sy, g.Hc, g.S);
  for (int i = 0; i < g.nx; ++i) ox[i] = tile_origin(i, g.sx, g.Wc, g.S);
  return 0;
}

int64_t mi355_tiled_workspace_bytes(const mi355_unet* net, int batch, const mi355_tile_plan* plan) {
  TileSpec ts;
  if (int rc = check_tile_plan("tiled_workspace_bytes", net, plan, batch, ts)) return rc;
  LayoutSpec sp = plain_spec(plan->chunk);
  sp.tile = &ts;
  return layout_bytes(net, sp);
}

int mi355_tile_gather(const float* canvas, float* windows, int batch, int channels, int image_size, const mi355_tile_plan* plan, void* stream) {
  TileGeom g;
  if (int rc = tile_geom(image_size, plan, &g, "tile_gather")) return rc;
  return tile_gather_launch(canvas, windows, batch, channels, g, S(stream));
}

int mi355_tile_labels(const int32_t* labels, int32_t* out, int batch, int n_windows, void* stream) {
  return tile_labels_launch(labels, out, batch, n_windows, S(stream));
}

int mi355_tile_blend(const float* windows, float* vbar, float* euler_x, float dt, int batch, int channels, int image_size, const mi355_tile_plan* plan,
                     void* stream) {
  TileGeom g;
  if (int rc = tile_geom(image_size, plan, &g, "tile_blend")) return rc;
  return tile_blend_launch(windows, vbar, euler_x, dt, batch, channels, g, S(stream));
}

int mi355_unet_forward_tiled(mi355_unet* net, const float* x, int x_channels, const float* cond, int cond_channels, float t_host, const int32_t* labels,
                             float* out, int batch, const mi355_tile_plan* plan, void* workspace, int64_t workspace_bytes, void* stream) {
  const char* const who = "unet_forward_tiled";
  TileSpec ts;
  if (int rc = check_tile_plan(who, net, plan, batch, ts)) return rc;
  MI355_REQUIRE(x && out, -1, "unet_forward_tiled: x or out is null");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "unet_forward_tiled: class labels given to a net built without num_classes");
  MI355_REQUIRE(x_channels > 0 && x_channels + (cond ? cond_channels : 0) == net->cfg.in_channels, -2,
                "unet_forward_tiled: x_channels and cond_channels do not add up to in_channels");
  LayoutSpec spec = plain_spec(plan->chunk);
  spec.tile = &ts;
  Layout l;
  if (int rc = carve(net, spec, workspace, workspace_bytes, l, who)) return rc;
  hipStream_t s = S(stream);
  TiledEval te = tiled_eval(ts, plan->chunk, l);
  if (cond) { if (int rc = te.gather_cond(cond, x_channels, cond_channels, s)) return rc; }
  if (labels) { if (int rc = te.repeat_labels(labels, s)) return rc; }
  if (int rc = fill_launch(l.sc.t, t_host, plan->chunk, s)) return rc;
  if (int rc = te.eval(net, l.sc, uniform_t_run(), x, x_channels, cond ? te.cond_windows(x_channels) : nullptr, cond_channels, false, nullptr, 0.f, s)) return rc;
  const int64_t n = (int64_t)batch * net->cfg.out_channels * ts.g.Hc * ts.g.Wc;
  MI355_CHECK_HIP(hipMemcpyAsync(out, l.tile.vbar, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  return 0;
}

int mi355_cfm_euler_sample_tiled(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, int cond_drift,
                                 const int32_t* labels, const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch,
                                 void* workspace, int64_t workspace_bytes, void* stream, const mi355_tile_plan* plan) {
  MI355_REQUIRE(net && x && t_span_host && n_t >= 1, -1, "cfm_euler_sample_tiled: bad argument");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "cfm_euler_sample_tiled: class labels given to a net built without num_classes");
  MI355_REQUIRE(x_channels == net->cfg.out_channels, -2, "cfm_euler_sample_tiled: the vector field must have the state's channel count");
  const char* const who = "cfm_euler_sample_tiled";
  TileSpec ts;
  if (int rc = check_tile_plan(who, net, plan, batch, ts)) return rc;
  MI355_REQUIRE(!cond_drift, -4, "cfm_euler_sample_tiled: cond_drift (the drifting condition of the concatenated-state sampler) is not built under tiling");
  MI355_REQUIRE(x_channels + (cond ? cond_channels : 0) == net->cfg.in_channels, -2,
                "cfm_euler_sample_tiled: x_channels and cond_channels do not add up to in_channels");
  LayoutSpec spec = plain_spec(plan->chunk);
  spec.tile = &ts;
  Layout l;
  if (int rc = carve(net, spec, workspace, workspace_bytes, l, who)) return rc;
  const Scratch& sc = l.sc;
  hipStream_t s = S(stream);
  TiledEval te = tiled_eval(ts, plan->chunk, l);
  EvalEmb emb;   // t_span_host is the caller's array: no wait
  if (int rc = emb.init(net, sc, t_span_host, n_t - 1, labels != nullptr, false, s)) return rc;
  const int64_t n = (int64_t)batch * x_channels * ts.g.Hc * ts.g.Wc;
  if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  if (cond) { if (int rc = te.gather_cond(cond, x_channels, cond_channels, s)) return rc; }
  if (labels) { if (int rc = te.repeat_labels(labels, s)) return rc; }
  if (int rc = cfm_euler_loop(net, sc, emb, x, x_channels, cond ? te.cond_windows(x_channels) : nullptr, cond_channels, nullptr, t_span_host, n_t, traj,
                              plan->chunk, n, 0, s, te.labels, nullptr, &te)) return rc;
  if (u8_out) return quantize_u8_launch(x, u8_out, n, s);
  return 0;
}

int mi355_ddpm_sample_tiled(mi355_unet* net, float* x, int channels, const float* cond, const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt,
                            const mi355_ddpm_schedule* sched, const float* noise, int64_t n_noise_draws, int batch, void* workspace,
                            int64_t workspace_bytes, void* stream, const mi355_tile_plan* plan) {
  MI355_REQUIRE(net && x && tb && opt, -1, "ddpm_sample_tiled: null argument");
  TileSpec ts;
  if (int rc = check_tile_plan("ddpm_sample_tiled", net, plan, batch, ts)) return rc;
  DdpmCall c = ddpm_call("ddpm_sample_tiled", plan->chunk, nullptr);   // the net runs at the chunk
  if (sched) {
    if (int rc = check_schedule(c.who, tb, opt, sched, false, c.ls)) return rc;
    c.th = sched_times(tb->Ns, sched);
  } else {
    c.th = ddpm_times(tb->Ns);
  }
  c.tile = &ts; c.spec.tile = &ts;
  return ddpm_run(c, net, x, channels, cond, tb, opt, noise, n_noise_draws, workspace, workspace_bytes, stream);
}

}  // extern "C"
