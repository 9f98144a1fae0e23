// extern "C" boundary of libmi355_sampler.so (see include/mi355_sampler.h) and the sampler loops.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "unet_engine.h"

static thread_local std::string g_err;
void mi355_set_error(const std::string& msg) { g_err = msg; }

namespace {
inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
}  // namespace

// The sampler loops know every step time in advance: all emb_layers outputs of up to EMB_TABLE_STEPS steps are computed by four
// launches before the loop instead of four launches per step (longer schedules fall back to the per-step path).
constexpr int EMB_TABLE_STEPS = 1024;
static size_t emb_table_bytes(const mi355_unet* net) {
  return al256((size_t)EMB_TABLE_STEPS * 4) + al256((size_t)EMB_TABLE_STEPS * ((size_t)net->emb_total + 9 * (size_t)net->cfg.model_channels) * 4);
}

static UnetRun uniform_t_run();

const mi355_debug_config& mi355_default_debug() {
  static const mi355_debug_config d = [] { mi355_debug_config c; mi355_debug_defaults(&c); return c; }();
  return d;
}

extern "C" {

int mi355_version(void) { return 107; }
void mi355_debug_defaults(mi355_debug_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->conv_ws = 1; c->conv_small = 15; c->conv_min_wgs = 512; c->conv_stagger = 0; c->conv_ablate = 0; c->conv_spin_limit = 1 << 22;
  c->conv_time_reps = 0; c->gn_apply_max_hw = 64; c->gn_fuse = 1; c->l2_warm = 1; c->attn_fused = 1; c->gn_epilogue = 7; c->conv_pp = 109; c->conv_edge = 15;
}
int mi355_unet_status(mi355_unet* net, int clear) {
  if (!net) { mi355_set_error("null handle"); return -1; }
  return unet_status(net, clear);
}
const char* mi355_last_error(void) { return g_err.c_str(); }

int mi355_unet_param_count(const mi355_unet_config* cfg) {
  if (!cfg) { mi355_set_error("null config"); return -1; }
  std::vector<ParamInfo> p;
  int rc = unet_enumerate_params(*cfg, p);
  return rc ? rc : (int)p.size();
}

int mi355_unet_param_info(const mi355_unet_config* cfg, int index, char* name, int name_cap, int64_t shape[4], int* ndim) {
  if (!cfg || !name || !shape || !ndim) { mi355_set_error("null argument"); return -1; }
  std::vector<ParamInfo> p;
  if (int rc = unet_enumerate_params(*cfg, p)) return rc;
  MI355_REQUIRE(index >= 0 && index < (int)p.size(), -1, "param index out of range");
  MI355_REQUIRE((int)p[index].name.size() + 1 <= name_cap, -1, "name buffer too small");
  std::strcpy(name, p[index].name.c_str());
  *ndim = (int)p[index].shape.size();
  for (int i = 0; i < 4; ++i) shape[i] = i < *ndim ? p[index].shape[i] : 1;
  return 0;
}

int64_t mi355_unet_weight_bytes(const mi355_unet_config* cfg) {
  if (!cfg) { mi355_set_error("null config"); return -1; }
  return unet_weight_bytes(*cfg);
}

int mi355_unet_create(const mi355_unet_config* cfg, const float* const* params_host, int n_params, void* dev_weights,
                      int64_t dev_weights_bytes, void* stream, mi355_unet** out) {
  if (!cfg) { mi355_set_error("null config"); return -1; }
  return unet_build(*cfg, params_host, n_params, dev_weights, dev_weights_bytes, S(stream), out);
}

void mi355_unet_destroy(mi355_unet* net) { delete net; }

int64_t mi355_unet_workspace_bytes(const mi355_unet* net, int batch) {
  if (!net || batch <= 0) { mi355_set_error("bad argument"); return -1; }
  // + sampler scratch: t[B], eps/v [B,Cout,H,W], none_like [B,Cin,H,W], and the per-step time-embedding table of the sampler loops
  const size_t hw = (size_t)net->cfg.image_size * net->cfg.image_size;
  // (+ the graph form's resident state [B,Cout,H,W], mi355_debug_config::sampler_graph)
  const size_t scratch = al256((size_t)batch * 4) + 2 * al256((size_t)batch * 32 * hw * 4) + emb_table_bytes(net) +
                         al256((size_t)batch * net->cfg.out_channels * hw * 4);
  return unet_workspace_bytes(net, batch) + (int64_t)scratch;
}

int mi355_unet_forward(mi355_unet* net, const float* x, int x_channels, const float* cond, int cond_channels, const float* t,
                       float* out, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  return unet_forward(net, x, x_channels, cond, cond_channels, t, out, batch, workspace, workspace_bytes, S(stream));
}

int mi355_unet_forward_t(mi355_unet* net, const float* x, int x_channels, const float* cond, int cond_channels, float t, float* out,
                         int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && workspace && batch > 0, -1, "unet_forward_t: bad argument");
  const WsLayout l = unet_ws_layout(net, batch);
  MI355_REQUIRE((int64_t)l.total <= workspace_bytes, -2, "unet_forward_t: workspace too small");
  // the step time lives in the first word of the workspace's emb2 region until the embedding kernels have read it (they write
  // temb -> emb1 -> emb2 in that order, t is read by the first one only); every image shares it: ONE embedding row
  float* tdev = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + l.emb2);
  if (int rc = fill_launch(tdev, t, 1, S(stream))) return rc;
  return unet_forward(net, x, x_channels, cond, cond_channels, tdev, out, batch, workspace, workspace_bytes, S(stream), uniform_t_run());
}

int mi355_unet_forward_labels(mi355_unet* net, const float* x, int x_channels, const float* cond, int cond_channels, const float* t, float t_host,
                              const int32_t* labels, float* out, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && workspace && batch > 0, -1, "unet_forward_labels: bad argument");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "unet_forward_labels: class labels given to a net built without num_classes");
  UnetRun run;
  run.labels = labels;
  if (!t) {   // one host time for the batch: staged as in mi355_unet_forward_t
    const WsLayout l = unet_ws_layout(net, batch);
    MI355_REQUIRE((int64_t)l.total <= workspace_bytes, -2, "unet_forward_labels: workspace too small");
    float* tdev = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + l.emb2);
    if (int rc = fill_launch(tdev, t_host, 1, S(stream))) return rc;
    t = tdev;
    run.t_uniform = 1;
  }
  return unet_forward(net, x, x_channels, cond, cond_channels, t, out, batch, workspace, workspace_bytes, S(stream), run);
}

int mi355_unet_vjp(mi355_unet* net, const float* grad_out, float* grad_x, int x_channels, int batch, void* workspace, int64_t workspace_bytes,
                   void* stream) {
  MI355_REQUIRE(net && workspace, -1, "unet_vjp: null argument");
  // same layout as mi355_unet_forward: the engine workspace starts at `workspace` (only the sampler loops carve their scratch in front)
  const int64_t engine_bytes = unet_workspace_bytes(net, batch);
  MI355_REQUIRE(workspace_bytes >= engine_bytes, -2, "unet_vjp: workspace too small");
  return unet_backward(net, grad_out, grad_x, x_channels, batch, workspace, workspace_bytes, S(stream));
}

int mi355_unet_plan_op(const mi355_unet* net, int index, int32_t fields[16]) {
  MI355_REQUIRE(net && fields, -1, "plan_op: null argument");
  if (index < 0 || index >= (int)net->ops.size()) return -1;
  const PlanOp& o = net->ops[index];
  const int32_t v[16] = {o.kind, o.src0, o.src1, o.dst, o.mode, o.ks, o.Cout, o.use_pro, o.pro_silu, o.res, o.res_mode, o.gn_site, o.heads, o.ch,
                         o.dst >= 0 ? net->tensors[o.dst].C : 0, o.dst >= 0 ? net->tensors[o.dst].H : 0};
  for (int i = 0; i < 16; ++i) fields[i] = v[i];
  return (int)net->ops.size();
}

int mi355_unet_read_tensor(const mi355_unet* net, int tensor, int gradient, float* out, int batch, void* workspace, int64_t workspace_bytes,
                           void* stream) {
  MI355_REQUIRE(net && out && workspace, -1, "read_tensor: null argument");
  MI355_REQUIRE(tensor >= 0 && tensor < (int)net->tensors.size(), -1, "read_tensor: tensor index out of range");
  MI355_REQUIRE(!gradient || net->cfg.differentiable, -4, "read_tensor: gradients exist in differentiable plans only");
  const WsLayout l = unet_ws_layout(net, batch);
  MI355_REQUIRE((int64_t)l.total <= workspace_bytes, -2, "read_tensor: workspace too small");
  const PlanTensor& t = net->tensors[tensor];
  const int tstate = (!gradient && (size_t)tensor < net->tensor_state_n) ? (int)net->tensor_state[tensor].load(std::memory_order_relaxed) : 0;
  if (tstate) {
    mi355_set_error(tstate == 1
                        ? "read_tensor: the last forward did not materialise this tensor (a conv output whose only reader, a GroupNorm site, ran in the conv's "
                          "epilogue; a 1x1 skip conv that rode in the next 3x3 conv; the packed network input the first conv read from the caller's tensor): "
                          "create the handle with debug.gn_epilogue = 0, conv_small = 7, conv_edge = 3 to inspect it"
                        : "read_tensor: the last forward normalised this conv output in place (16x16 level: it holds silu(GroupNorm(.)), not the conv's result): "
                          "create the handle with debug.gn_epilogue = 0 (or 1) to inspect it");
    return MI355_ERR_UNSUPPORTED;
  }
  const int esz = net->cfg.dtype == 0 ? 4 : 2;
  const char* p = reinterpret_cast<const char*>(workspace) + (gradient ? l.grads : l.arena) + t.offset_per_image * (size_t)batch * esz;
  return unpack_nchw_launch(net->cfg.dtype, p, batch, t.H * t.W, t.C, out, S(stream));
}

int mi355_unet_get_stats(const mi355_unet* net, int batch, mi355_unet_stats* out) {
  if (!net || !out) { mi355_set_error("null argument"); return -1; }
  out->launches = net->last_launches > 0 ? net->last_launches : net->launches;   // the most recent forward's real count once there was one
  out->conv_flops = net->conv_flops * batch;
  out->attn_flops = net->attn_flops * batch;
  out->act_bytes = net->act_bytes * batch;
  out->weight_bytes = net->weight_bytes;
  return 0;
}

int mi355_unet_profile(mi355_unet* net, const float* x, int x_channels, const float* cond, int cond_channels, const float* t,
                       float* out, int batch, void* workspace, int64_t workspace_bytes, void* stream, mi355_op_profile* recs,
                       int cap) {
  MI355_REQUIRE(net && recs && cap > 0, -1, "unet_profile: bad argument");
  std::vector<mi355_op_profile> prof;
  std::vector<hipEvent_t> ev;
  UnetRun run; run.prof = &prof; run.prof_events = &ev;
  int rc = unet_forward(net, x, x_channels, cond, cond_channels, t, out, batch, workspace, workspace_bytes, S(stream), run);
  // An event record is itself a packet the queue has to retire: an interval between two events holds one such gap besides the
  // op.  Calibrate it on this stream (back-to-back records with nothing in between) and take it off every interval, so the
  // per-op times agree with rocprofv3's kernel durations.
  constexpr int NCAL = 17;
  hipEvent_t cal[NCAL];
  for (int i = 0; i < NCAL; ++i) { (void)hipEventCreate(&cal[i]); (void)hipEventRecord(cal[i], S(stream)); }
  hipError_t e = hipStreamSynchronize(S(stream));
  if (rc == 0 && e == hipSuccess) {
    float gap = 0.f;
    for (int i = 0; i + 1 < NCAL; ++i) { float ms = 0.f; (void)hipEventElapsedTime(&ms, cal[i], cal[i + 1]); gap += ms; }
    gap /= (float)(NCAL - 1);
    for (size_t i = 0; i + 1 < ev.size() && i < prof.size(); ++i) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
      prof[i].ms = ms > 2.f * gap ? ms - gap : 0.5f * ms;
    }
  }
  for (int i = 0; i < NCAL; ++i) (void)hipEventDestroy(cal[i]);
  for (auto h : ev) (void)hipEventDestroy(h);
  if (rc) return rc;
  if (e != hipSuccess) { mi355_set_error(hipGetErrorString(e)); return -3; }
  const int n = (int)prof.size();
  for (int i = 0; i < n && i < cap; ++i) recs[i] = prof[i];
  return n;
}

// ---- sampler loops --------------------------------------------------------------------------------

struct Scratch { float* t; float* v; float* none; float* tsteps; float* embtab; float* xstate; char* unet_ws; int64_t unet_bytes; };
// every image of a sampler step shares the step time: the engine computes ONE embedding row (stride-0 broadcast)
static UnetRun uniform_t_run() { UnetRun r; r.t_uniform = 1; return r; }
// table[k] = emb_layers outputs for step time t_host[k] (k < n <= EMB_TABLE_STEPS); returns the table or null (per-step path).
// labelled (class-conditional sampling): table[k * K + c] = the rows of step k and class c, for n * K <= EMB_TABLE_STEPS rows
// (three time launches over n rows, one label_emb_linear over n * K); the steps gather their images' rows from it.
static int make_emb_table(const mi355_unet* net, const Scratch& sc, const float* t_host, int n, bool labelled, hipStream_t s, const float** table) {
  *table = nullptr;
  const int K = labelled ? net->num_classes : 1;
  if (n <= 0 || (int64_t)n * K > EMB_TABLE_STEPS) return 0;
  MI355_CHECK_HIP(hipMemcpyAsync(sc.tsteps, t_host, (size_t)n * 4, hipMemcpyHostToDevice, s));
  float* scratch = sc.embtab + (size_t)EMB_TABLE_STEPS * net->emb_total;
  if (int rc = labelled ? unet_embedding_rows_labels(net, sc.tsteps, n, nullptr, n * K, K, sc.embtab, scratch, s)
                        : unet_embedding_table(net, sc.tsteps, n, sc.embtab, scratch, s)) return rc;
  *table = sc.embtab;
  return 0;
}
static int carve(mi355_unet* net, int B, void* workspace, int64_t workspace_bytes, Scratch& sc) {
  MI355_REQUIRE(net && workspace, -1, "null argument");
  MI355_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 255) == 0, -1, "workspace must be 256-byte aligned");
  MI355_REQUIRE(workspace_bytes >= mi355_unet_workspace_bytes(net, B), -2, "workspace too small");
  const size_t hw = (size_t)net->cfg.image_size * net->cfg.image_size;
  char* p = reinterpret_cast<char*>(workspace);
  sc.t = reinterpret_cast<float*>(p); p += al256((size_t)B * 4);
  sc.v = reinterpret_cast<float*>(p); p += al256((size_t)B * 32 * hw * 4);
  sc.none = reinterpret_cast<float*>(p); p += al256((size_t)B * 32 * hw * 4);
  sc.tsteps = reinterpret_cast<float*>(p); p += al256((size_t)EMB_TABLE_STEPS * 4);
  sc.embtab = reinterpret_cast<float*>(p); p += al256((size_t)EMB_TABLE_STEPS * ((size_t)net->emb_total + 9 * (size_t)net->cfg.model_channels) * 4);
  sc.xstate = reinterpret_cast<float*>(p); p += al256((size_t)B * net->cfg.out_channels * hw * 4);
  sc.unet_ws = p;
  sc.unet_bytes = workspace_bytes - (p - reinterpret_cast<char*>(workspace));
  return 0;
}

// The loop proper: every launch of every step on stream s (the caller's stream, or the handle's capture stream while a graph is recorded).
// labels: class-conditional steps (with a table: step k's block of the (step, class) table, one gather launch per step).
static int cfm_euler_loop(mi355_unet* net, const Scratch& sc, float* x, int x_channels, const float* cond, int cond_channels, float* cdrift,
                          const float* t_span_host, int n_t, const float* emb_table, float* traj, int batch, int64_t n, int64_t nc, hipStream_t s,
                          const int32_t* labels = nullptr) {
  UnetRun run = uniform_t_run();
  run.labels = labels;
  const size_t block = (size_t)(labels ? net->num_classes : 1) * net->emb_total;
  for (int k = 0; k + 1 < n_t; ++k) {
    const float t = t_span_host[k], dt = t_span_host[k + 1] - t_span_host[k];
    int rc;
    if (emb_table) run.emb_row = emb_table + (size_t)k * block;
    else if ((rc = fill_launch(sc.t, t, batch, s))) return rc;
    run.euler_x = x; run.euler_dt = dt;   // x += dt * v: in the last conv's epilogue, or as a launch of unet_forward's own behind it
    if ((rc = unet_forward(net, x, x_channels, cond, cond_channels, sc.t, sc.v, batch, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
    if (cdrift && (rc = euler_step_launch(cdrift, cdrift, dt, nc, s))) return rc;
    if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj + (size_t)(k + 1) * n, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  }
  return 0;
}

// knobs.sampler_graph: the loop as ONE graph launch.  The graph works on the workspace's resident state (sc.xstate) so that it does not depend on
// the caller's x / u8 pointers (a fresh tensor per call is the normal use); it does depend on the workspace, the batch, the schedule (dt is a kernel
// argument, the embedding rows are table addresses) and the condition pointer: those are its key.  The embedding table is rebuilt on every call,
// outside the graph (the workspace is the caller's: another sampler may have used it in between).
static int cfm_euler_graph(mi355_unet* net, const Scratch& sc, float* x, int x_channels, const float* cond, int cond_channels, const float* t_span_host,
                           int n_t, const float* emb_table, int batch, int64_t n, void* workspace, hipStream_t s) {
  uint64_t h = 1469598103934665603ull;
  for (int k = 0; k < n_t; ++k) { uint32_t b; std::memcpy(&b, &t_span_host[k], 4); h = (h ^ b) * 1099511628211ull; }
  const uint64_t key[8] = {(uint64_t)reinterpret_cast<uintptr_t>(workspace), (uint64_t)batch, (uint64_t)n_t, h, (uint64_t)reinterpret_cast<uintptr_t>(cond),
                           (uint64_t)cond_channels, (uint64_t)x_channels, (uint64_t)reinterpret_cast<uintptr_t>(emb_table)};
  std::lock_guard<std::mutex> lock(net->graph_mu);
  mi355_unet::SamplerGraph* g = nullptr;
  for (auto& e : net->graphs) if (e.exec && std::memcmp(e.key, key, sizeof(key)) == 0) { g = &e; break; }
  if (!g) {
    if (!net->capture_stream) MI355_CHECK_HIP(hipStreamCreateWithFlags(&net->capture_stream, hipStreamNonBlocking));
    hipStream_t cs = net->capture_stream;
    MI355_CHECK_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal));
    int rc = cfm_euler_loop(net, sc, sc.xstate, x_channels, cond, cond_channels, nullptr, t_span_host, n_t, emb_table, nullptr, batch, n, 0, cs);
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

int mi355_cfm_euler_sample(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, int cond_drift,
                           const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch, void* workspace,
                           int64_t workspace_bytes, void* stream) {
  return mi355_cfm_euler_sample_labels(net, x, x_channels, cond, cond_channels, cond_drift, nullptr, t_span_host, n_t, traj, u8_out, batch,
                                       workspace, workspace_bytes, stream);
}

int mi355_cfm_euler_sample_labels(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, int cond_drift,
                                  const int32_t* labels, const float* t_span_host, int n_t, float* traj, uint8_t* u8_out, int batch,
                                  void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && t_span_host && n_t >= 1, -1, "cfm_euler_sample: bad argument");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "cfm_euler_sample: class labels given to a net built without num_classes");
  MI355_REQUIRE(x_channels == net->cfg.out_channels, -2, "cfm_euler_sample: the vector field must have the state's channel count");
  Scratch sc;
  if (int rc = carve(net, batch, workspace, workspace_bytes, sc)) return rc;
  hipStream_t s = S(stream);
  const float* emb_table = nullptr;
  if (int rc = make_emb_table(net, sc, t_span_host, n_t - 1, labels != nullptr, s, &emb_table)) return rc;
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
  if (net->knobs.sampler_graph && emb_table && !traj && !cdrift && !labels && n_t > 1)
    rc = cfm_euler_graph(net, sc, x, x_channels, cond, cond_channels, t_span_host, n_t, emb_table, batch, n, workspace, s);
  else
    rc = cfm_euler_loop(net, sc, x, x_channels, cond, cond_channels, cdrift, t_span_host, n_t, emb_table, traj, batch, n, nc, s, labels);
  if (rc) return rc;
  if (u8_out) return quantize_u8_launch(x, u8_out, n, s);
  return 0;
}

// Fixed-step explicit Runge-Kutta CFM sampler over a general tableau (midpoint, Heun, RK4, ...).  The stage derivatives k_1..k_s and the stage state
// live behind the network workspace: (stages + 1) state-sized buffers.
static size_t rk_state_bytes(const mi355_unet* net, int batch) {
  return al256((size_t)batch * net->cfg.out_channels * net->cfg.image_size * net->cfg.image_size * 4);
}
// t + c * dt with the product and the sum each rounded to fp32 (c == 0 / 1: the interval's end points themselves, as mi355/ode.py's dopri5 does)
static float rk_stage_time(float t0, float t1, float c) {
#pragma clang fp contract(off)
  if (c == 0.f) return t0;
  if (c == 1.f) return t1;
  const float dt = t1 - t0;
  const float p = c * dt;
  return t0 + p;
}

int64_t mi355_cfm_rk_workspace_bytes(const mi355_unet* net, int batch, int stages) {
  if (!net || batch <= 0 || stages < 1 || stages > 4) { mi355_set_error("cfm_rk_workspace_bytes: bad argument (1 <= stages <= 4)"); return -1; }
  return (int64_t)al256((size_t)mi355_unet_workspace_bytes(net, batch)) + (int64_t)(stages + 1) * (int64_t)rk_state_bytes(net, batch);
}

int mi355_cfm_rk_sample(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, const int32_t* labels,
                        const float* t_span_host, int n_t, int stages, const float* a_host, const float* b_host, const float* c_host, float* traj,
                        uint8_t* u8_out, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && t_span_host && n_t >= 1 && batch > 0, -1, "cfm_rk_sample: bad argument");
  MI355_REQUIRE(stages >= 1 && stages <= 4, -1, "cfm_rk_sample: the tableau must have 1 to 4 stages");
  MI355_REQUIRE(a_host && b_host && c_host, -1, "cfm_rk_sample: null tableau");
  bool any_b = false;
  for (int j = 0; j < stages; ++j) any_b = any_b || b_host[j] != 0.f;
  MI355_REQUIRE(any_b, -1, "cfm_rk_sample: the tableau's weights b are all zero");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "cfm_rk_sample: class labels given to a net built without num_classes");
  MI355_REQUIRE(x_channels == net->cfg.out_channels, -2, "cfm_rk_sample: the vector field must have the state's channel count");
  MI355_REQUIRE(workspace_bytes >= mi355_cfm_rk_workspace_bytes(net, batch, stages), -2, "cfm_rk_sample: workspace too small");
  const int64_t base = (int64_t)al256((size_t)mi355_unet_workspace_bytes(net, batch));
  Scratch sc;
  if (int rc = carve(net, batch, workspace, base, sc)) return rc;
  hipStream_t s = S(stream);
  const int64_t n = (int64_t)batch * x_channels * net->cfg.image_size * net->cfg.image_size;
  float* kbuf[4] = {nullptr, nullptr, nullptr, nullptr};
  char* tail = reinterpret_cast<char*>(workspace) + base;
  for (int i = 0; i < stages; ++i) kbuf[i] = reinterpret_cast<float*>(tail + (size_t)i * rk_state_bytes(net, batch));
  float* ystage = reinterpret_cast<float*>(tail + (size_t)stages * rk_state_bytes(net, batch));
  if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  const int n_steps = n_t - 1;
  if (n_steps == 0) return u8_out ? quantize_u8_launch(x, u8_out, n, s) : 0;
  // every evaluation time is known in advance: one embedding row (block of num_classes rows with labels) per (step, stage)
  std::vector<float> te((size_t)n_steps * stages);
  for (int k = 0; k < n_steps; ++k)
    for (int i = 0; i < stages; ++i) te[(size_t)k * stages + i] = rk_stage_time(t_span_host[k], t_span_host[k + 1], c_host[i]);
  // The rule is rows = n_steps * stages * K <= EMB_TABLE_STEPS (K = num_classes with labels, else 1), and make_emb_table applies it: beyond
  // it the table stays null and every evaluation computes its own rows.  The test here leaves K out on purpose: it only keeps the row
  // count that is handed over within an int and within sc.tsteps.
  const float* emb_table = nullptr;
  if ((int64_t)n_steps * stages <= EMB_TABLE_STEPS) {
    if (int rc = make_emb_table(net, sc, te.data(), n_steps * stages, labels != nullptr, s, &emb_table)) return rc;
    // `te` is a temporary host buffer: wait for its copy, once per call, as ddpm_sample and sf2m_euler_sample do (no graph capture here)
    if (emb_table) MI355_CHECK_HIP(hipStreamSynchronize(s));
  }
  UnetRun run = uniform_t_run();   // no euler_x: the last conv stores v (conv_edge bit 3 stays out of these evaluations)
  run.labels = labels;
  const size_t block = (size_t)(labels ? net->num_classes : 1) * net->emb_total;
  int rc = 0;
  for (int k = 0; k < n_steps; ++k) {
    const float dt = t_span_host[k + 1] - t_span_host[k];
    for (int i = 0; i < stages; ++i) {
      // y_i = x + sum_{j<i} (dt * a_ij) k_j over the non-zero a_ij; none: the stage reads x itself
      const float* kp[4]; float cf[4]; int nk = 0;
      for (int j = 0; j < i; ++j) {
        const float a = a_host[(size_t)i * stages + j];
        if (a != 0.f) { kp[nk] = kbuf[j]; cf[nk] = dt * a; ++nk; }
      }
      const float* yin = x;
      if (nk) { if ((rc = rk_stage_launch(ystage, x, kp, cf, nk, n, nullptr, nullptr, s))) return rc; yin = ystage; }
      const size_t e = (size_t)k * stages + i;
      if (emb_table) run.emb_row = emb_table + e * block;
      else if ((rc = fill_launch(sc.t, te[e], batch, s))) return rc;
      if ((rc = unet_forward(net, yin, x_channels, cond, cond_channels, sc.t, kbuf[i], batch, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
    }
    const float* kp[4]; float cf[4]; int nk = 0;
    for (int j = 0; j < stages; ++j)
      if (b_host[j] != 0.f) { kp[nk] = kbuf[j]; cf[nk] = dt * b_host[j]; ++nk; }   // nk >= 1: an all-zero b was refused above
    // the step's update, in place, with the trajectory slot and (last step) the image bytes from the same launch
    if ((rc = rk_stage_launch(x, x, kp, cf, nk, n, traj ? traj + (size_t)(k + 1) * n : nullptr, k + 1 == n_steps ? u8_out : nullptr, s))) return rc;
  }
  return 0;
}

int mi355_ddpm_sample(mi355_unet* net, float* x, int channels, const float* cond, const mi355_ddpm_tables* tb,
                      const mi355_ddpm_options* opt, const float* noise, int64_t n_noise_draws, int batch, void* workspace,
                      int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && tb && opt, -1, "ddpm_sample: null argument");
  MI355_REQUIRE(channels == net->cfg.out_channels, -2, "ddpm_sample: eps model must output the state's channel count");
  const int mode = opt->mode, Ns = tb->Ns;
  const bool amortized = net->cfg.in_channels == 2 * channels;
  MI355_REQUIRE(amortized || net->cfg.in_channels == channels, -2, "ddpm_sample: network in_channels must be C or 2C");
  MI355_REQUIRE(mode != MI355_DDPM_REPLACEMENT || (!amortized && cond), -2, "ddpm_sample: replacement needs an unconditional net and a condition");
  MI355_REQUIRE(mode != MI355_DDPM_AMORTIZED || (amortized && cond), -2, "ddpm_sample: amortized needs a 2C-input net and a condition");
  Scratch sc;
  if (int rc = carve(net, batch, workspace, workspace_bytes, sc)) return rc;
  UnetRun run = uniform_t_run();
  hipStream_t s = S(stream);
  const int64_t n = (int64_t)batch * channels * net->cfg.image_size * net->cfg.image_size;
  const int64_t n_al = (n + 3) / 4 * 4;
  int rc;
  const float* emb_table = nullptr;   // row i = step i (time i / Ns)
  if (Ns <= EMB_TABLE_STEPS) {
    std::vector<float> th((size_t)Ns);
    for (int i = 0; i < Ns; ++i) th[i] = (float)i / (float)Ns;
    if ((rc = make_emb_table(net, sc, th.data(), Ns, false, s, &emb_table))) return rc;
    MI355_CHECK_HIP(hipStreamSynchronize(s));   // `th` is a temporary host buffer (once per sample() call)
  }
  if (amortized && (rc = fill_launch(sc.none, opt->none_value, n, s))) return rc;
  // the net's condition input on predictor steps / on corrector steps (the reference's corrector calls
  // x0_model without the condition, sampling.py:116 -> none_like)
  const float* cond_pred = !amortized ? nullptr : ((mode == MI355_DDPM_AMORTIZED || (mode == MI355_DDIM && cond)) ? cond : sc.none);
  const float* cond_corr = amortized ? sc.none : nullptr;
  int64_t draw = 0;
  auto next_noise = [&](const float*& zptr, int& philox, uint64_t& off) -> int {
    if (noise) {
      MI355_REQUIRE(draw < n_noise_draws, -2, "ddpm_sample: injected noise exhausted");
      zptr = noise + (size_t)draw * n; philox = 0; off = 0;
    } else { zptr = nullptr; philox = 1; off = (uint64_t)draw * (uint64_t)n_al; }
    ++draw;
    return 0;
  };
  for (int i = Ns - 1; i >= 0; --i) {
    const float tval = (float)i / (float)Ns;  // eps_model(xi, i) = network(xi, 1.0*i/Ns)  loss_functions.py:18-19
    if (mode == MI355_DDPM_REPLACEMENT && i < (int)(Ns * opt->start_fraction)) {
      const float* z = nullptr; int ph = 0; uint64_t off = 0;
      if (opt->noise_condition && (rc = next_noise(z, ph, off))) return rc;
      if ((rc = replace_mask_launch(x, cond, z, opt->pad_value, opt->noise_condition, tb->sqrt_alphas_cumprod[i],
                                    tb->sqrt_one_minus_alphas_cumprod[i], ph, opt->seed, off, n, s))) return rc;
    }
    if (emb_table) run.emb_row = emb_table + (size_t)i * net->emb_total;
    else if ((rc = fill_launch(sc.t, tval, batch, s))) return rc;
    if ((rc = unet_forward(net, x, channels, cond_pred, channels, sc.t, sc.v, batch, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
    if (mode == MI355_DDIM) {
      if ((rc = ddim_step_launch(x, sc.v, tb->sqrt_recip_alphas_cumprod[i], tb->sqrt_recipm1_alphas_cumprod[i],
                                 tb->alphas_cumprod_prev[i], n, s))) return rc;
      continue;
    }
    const float* z = nullptr; int ph = 0; uint64_t off = 0;
    if (i > 0 && (rc = next_noise(z, ph, off))) return rc;
    const float sigma = expf(0.5f * tb->posterior_log_variance_clipped[i]);
    if ((rc = ddpm_step_launch(x, sc.v, z, tb->sqrt_recip_alphas_cumprod[i], tb->sqrt_recipm1_alphas_cumprod[i],
                               tb->posterior_mean_coef1[i], tb->posterior_mean_coef2[i], sigma, ph, opt->seed, off, n, s))) return rc;
    for (int c = 0; c < opt->n_corrector; ++c) {
      if ((rc = unet_forward(net, x, channels, cond_corr, channels, sc.t, sc.v, batch, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
      const float* z2 = nullptr; int ph2 = 0; uint64_t off2 = 0;
      if ((rc = next_noise(z2, ph2, off2))) return rc;
      const float dt = (opt->tmax - opt->tmin) / (float)Ns;
      if ((rc = corrector_step_launch(x, sc.v, z2, tb->sqrt_recip_alphas_cumprod[i], tb->sqrt_recipm1_alphas_cumprod[i],
                                      tb->recip_sqrt_m1_alphas_cumprod[i], dt, opt->delta, ph2, opt->seed, off2, n, s))) return rc;
    }
  }
  return clip_launch(x, -1.f, 1.f, n, s);
}

// ---- classifier-free guidance: every evaluation is ONE forward at batch 2B (images 0..B-1 conditional, B..2B-1 unconditional) -------------------
namespace {
// the buffers behind the 2B network workspace: duplicated state, condition | none, labels | null, then the CFM sampler's stage buffers
struct CfgTail { float* x2; float* cond2; int32_t* labels2; char* rest; };
inline size_t cfg_cond_channels(const mi355_unet* net) { return (size_t)(net->cfg.in_channels > net->cfg.out_channels ? net->cfg.in_channels - net->cfg.out_channels : 0); }
inline size_t cfg_state2_bytes(const mi355_unet* net, int batch) {
  return al256((size_t)2 * batch * net->cfg.out_channels * net->cfg.image_size * net->cfg.image_size * 4);
}
inline size_t cfg_cond2_bytes(const mi355_unet* net, int batch) {
  const size_t cc = cfg_cond_channels(net);
  return cc ? al256((size_t)2 * batch * cc * net->cfg.image_size * net->cfg.image_size * 4) : 0;
}
inline size_t cfg_labels2_bytes(const mi355_unet* net, int batch) { return net->num_classes > 0 ? al256((size_t)2 * batch * 4) : 0; }
inline size_t cfg_tail_bytes(const mi355_unet* net, int batch) { return cfg_state2_bytes(net, batch) + cfg_cond2_bytes(net, batch) + cfg_labels2_bytes(net, batch); }
inline CfgTail cfg_tail(const mi355_unet* net, int batch, char* p) {
  CfgTail t;
  t.x2 = reinterpret_cast<float*>(p); p += cfg_state2_bytes(net, batch);
  t.cond2 = reinterpret_cast<float*>(p); p += cfg_cond2_bytes(net, batch);
  t.labels2 = reinterpret_cast<int32_t*>(p); p += cfg_labels2_bytes(net, batch);
  t.rest = p;
  return t;
}
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
}  // namespace

int64_t mi355_cfg_workspace_bytes(const mi355_unet* net, int batch, int stages) {
  if (!net || batch <= 0 || stages < 1 || stages > 4) { mi355_set_error("cfg_workspace_bytes: bad argument (1 <= stages <= 4)"); return -1; }
  return (int64_t)al256((size_t)mi355_unet_workspace_bytes(net, 2 * batch)) + (int64_t)cfg_tail_bytes(net, batch) +
         (int64_t)(stages + (stages > 1 ? 1 : 0)) * (int64_t)cfg_state2_bytes(net, batch);
}

int64_t mi355_ddpm_cfg_workspace_bytes(const mi355_unet* net, int batch) {
  if (!net || batch <= 0) { mi355_set_error("ddpm_cfg_workspace_bytes: bad argument"); return -1; }
  return (int64_t)al256((size_t)mi355_unet_workspace_bytes(net, 2 * batch)) + (int64_t)cfg_tail_bytes(net, batch);
}

int mi355_cfm_cfg_sample(mi355_unet* net, float* x, int x_channels, const float* cond, int cond_channels, float none_value, const int32_t* labels,
                         int null_label, float w, const float* w_dev, const float* t_span_host, int n_t, int stages, const float* a_host,
                         const float* b_host, const float* c_host, float* traj, uint8_t* u8_out, int batch, void* workspace, int64_t workspace_bytes,
                         void* stream) {
  MI355_REQUIRE(net && x && t_span_host && n_t >= 1 && batch > 0, -1, "cfm_cfg_sample: bad argument");
  MI355_REQUIRE(stages >= 1 && stages <= 4, -1, "cfm_cfg_sample: the tableau must have 1 to 4 stages");
  MI355_REQUIRE(a_host && b_host && c_host, -1, "cfm_cfg_sample: null tableau");
  bool any_b = false;
  for (int j = 0; j < stages; ++j) any_b = any_b || b_host[j] != 0.f;
  MI355_REQUIRE(any_b, -1, "cfm_cfg_sample: the tableau's weights b are all zero");
  MI355_REQUIRE(cond || labels, -1, "cfm_cfg_sample: nothing to guide (neither a condition nor class labels)");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "cfm_cfg_sample: class labels given to a net built without num_classes");
  MI355_REQUIRE(!labels || (null_label >= 0 && null_label < net->num_classes), -1, "cfm_cfg_sample: null_label must be a class index in [0, num_classes)");
  MI355_REQUIRE(x_channels == net->cfg.out_channels, -2, "cfm_cfg_sample: the vector field must have the state's channel count");
  MI355_REQUIRE(!cond || (cond_channels > 0 && (size_t)cond_channels == cfg_cond_channels(net)), -2,
                "cfm_cfg_sample: the condition must have in_channels - out_channels channels");
  MI355_REQUIRE(workspace_bytes >= mi355_cfg_workspace_bytes(net, batch, stages), -2, "cfm_cfg_sample: workspace too small");
  const int B2 = 2 * batch;
  const int64_t base = (int64_t)al256((size_t)mi355_unet_workspace_bytes(net, B2));
  Scratch sc;
  if (int rc = carve(net, B2, workspace, base, sc)) return rc;
  hipStream_t s = S(stream);
  const int64_t hw = (int64_t)net->cfg.image_size * net->cfg.image_size;
  const int64_t per = (int64_t)x_channels * hw, n = (int64_t)batch * per, nc = (int64_t)batch * cond_channels * hw;
  const CfgTail tl = cfg_tail(net, batch, reinterpret_cast<char*>(workspace) + base);
  float* kbuf[4] = {nullptr, nullptr, nullptr, nullptr};
  for (int i = 0; i < stages; ++i) kbuf[i] = reinterpret_cast<float*>(tl.rest + (size_t)i * cfg_state2_bytes(net, batch));
  float* ystage = reinterpret_cast<float*>(tl.rest + (size_t)stages * cfg_state2_bytes(net, batch));   // (stages > 1 only)
  if (traj) MI355_CHECK_HIP(hipMemcpyAsync(traj, x, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  const int n_steps = n_t - 1;
  if (n_steps == 0) return u8_out ? quantize_u8_launch(x, u8_out, n, s) : 0;
  if (int rc = cfg_fill_tail(tl, x, n, cond, nc, none_value, labels, null_label, batch, s)) return rc;
  std::vector<float> te((size_t)n_steps * stages);
  for (int k = 0; k < n_steps; ++k)
    for (int i = 0; i < stages; ++i) te[(size_t)k * stages + i] = rk_stage_time(t_span_host[k], t_span_host[k + 1], c_host[i]);
  // rows = n_steps * stages * K <= EMB_TABLE_STEPS (make_emb_table applies it), as in mi355_cfm_rk_sample
  const float* emb_table = nullptr;
  if ((int64_t)n_steps * stages <= EMB_TABLE_STEPS) {
    if (int rc = make_emb_table(net, sc, te.data(), n_steps * stages, labels != nullptr, s, &emb_table)) return rc;
    if (emb_table) MI355_CHECK_HIP(hipStreamSynchronize(s));   // `te` is a temporary host buffer: once per call
  }
  UnetRun run = uniform_t_run();
  run.labels = labels ? tl.labels2 : nullptr;
  const float* cond2 = cond ? tl.cond2 : nullptr;
  const size_t block = (size_t)(labels ? net->num_classes : 1) * net->emb_total;
  int64_t step_launches = 0;
  int rc = 0;
  for (int k = 0; k < n_steps; ++k) {
    const float dt = t_span_host[k + 1] - t_span_host[k];
    step_launches = 0;
    for (int i = 0; i < stages; ++i) {
      const float* kp[4]; float cf[4]; int nk = 0;
      for (int j = 0; j < i; ++j) {
        const float a = a_host[(size_t)i * stages + j];
        if (a != 0.f) { kp[nk] = kbuf[j]; cf[nk] = dt * a; ++nk; }
      }
      const float* yin = tl.x2;
      if (nk) {   // the stage state, both halves
        if ((rc = cfg_stage_launch(ystage, tl.x2, kp, cf, nk, n, w, w_dev, per, 1, nullptr, nullptr, s))) return rc;
        yin = ystage; ++step_launches;
      }
      const size_t e = (size_t)k * stages + i;
      if (emb_table) run.emb_row = emb_table + e * block;
      else { if ((rc = fill_launch(sc.t, te[e], B2, s))) return rc; ++step_launches; }
      if ((rc = unet_forward(net, yin, x_channels, cond2, cond_channels, sc.t, kbuf[i], B2, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
      step_launches += net->last_launches;
    }
    const float* kp[4]; float cf[4]; int nk = 0;
    for (int j = 0; j < stages; ++j)
      if (b_host[j] != 0.f) { kp[nk] = kbuf[j]; cf[nk] = dt * b_host[j]; ++nk; }
    // the update: both halves of x2 in place, the trajectory slot and (last step) the image bytes from the same launch
    if ((rc = cfg_stage_launch(tl.x2, tl.x2, kp, cf, nk, n, w, w_dev, per, 1, traj ? traj + (size_t)(k + 1) * n : nullptr,
                               k + 1 == n_steps ? u8_out : nullptr, s))) return rc;
    ++step_launches;
  }
  MI355_CHECK_HIP(hipMemcpyAsync(x, tl.x2, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
  net->last_launches = step_launches;   // mi355_unet_get_stats: every launch of the last step (evaluations and stage launches)
  return 0;
}

int mi355_ddpm_cfg_sample(mi355_unet* net, float* x, int channels, const float* cond, const int32_t* labels, int null_label, float w, const float* w_dev,
                          const mi355_ddpm_tables* tb, const mi355_ddpm_options* opt, const float* noise, int64_t n_noise_draws, int batch,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  MI355_REQUIRE(net && x && tb && opt && batch > 0, -1, "ddpm_cfg_sample: bad argument");
  const int mode = opt->mode, Ns = tb->Ns;
  MI355_REQUIRE(mode == MI355_DDPM_AMORTIZED || mode == MI355_DDIM, -1,
                "ddpm_cfg_sample: guidance is built for the amortized sampler and for DDIM with a condition (prior and replacement modes are refused)");
  MI355_REQUIRE(cond || labels, -1, "ddpm_cfg_sample: nothing to guide (neither a condition nor class labels)");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, "ddpm_cfg_sample: class labels given to a net built without num_classes");
  MI355_REQUIRE(!labels || (null_label >= 0 && null_label < net->num_classes), -1, "ddpm_cfg_sample: null_label must be a class index in [0, num_classes)");
  MI355_REQUIRE(channels == net->cfg.out_channels, -2, "ddpm_cfg_sample: eps model must output the state's channel count");
  MI355_REQUIRE(net->cfg.in_channels == 2 * channels && cond, -2, "ddpm_cfg_sample: needs a 2C-input net and a condition");
  MI355_REQUIRE(workspace_bytes >= mi355_ddpm_cfg_workspace_bytes(net, batch), -2, "ddpm_cfg_sample: workspace too small");
  const int B2 = 2 * batch;
  const int64_t base = (int64_t)al256((size_t)mi355_unet_workspace_bytes(net, B2));
  Scratch sc;
  if (int rc = carve(net, B2, workspace, base, sc)) return rc;
  hipStream_t s = S(stream);
  const int64_t per = (int64_t)channels * net->cfg.image_size * net->cfg.image_size, n = (int64_t)batch * per;
  const int64_t n_al = (n + 3) / 4 * 4;
  const CfgTail tl = cfg_tail(net, batch, reinterpret_cast<char*>(workspace) + base);
  int rc;
  const float* emb_table = nullptr;   // row i (block of num_classes rows with labels) = step i (time i / Ns)
  if (Ns <= EMB_TABLE_STEPS) {
    std::vector<float> th((size_t)Ns);
    for (int i = 0; i < Ns; ++i) th[i] = (float)i / (float)Ns;
    if ((rc = make_emb_table(net, sc, th.data(), Ns, labels != nullptr, s, &emb_table))) return rc;
    MI355_CHECK_HIP(hipStreamSynchronize(s));   // `th` is a temporary host buffer (once per call)
  }
  if ((rc = cfg_fill_tail(tl, x, n, cond, n, opt->none_value, labels, null_label, batch, s))) return rc;
  UnetRun run = uniform_t_run(), run_corr = uniform_t_run();
  run.labels = labels ? tl.labels2 : nullptr;
  run_corr.labels = labels ? tl.labels2 + batch : nullptr;   // the corrector sees no condition (sampling.py:116): none_like and the null label
  const size_t block = (size_t)(labels ? net->num_classes : 1) * net->emb_total;
  int64_t draw = 0;
  auto next_noise = [&](const float*& zptr, int& philox, uint64_t& off) -> int {
    if (noise) {
      MI355_REQUIRE(draw < n_noise_draws, -2, "ddpm_cfg_sample: injected noise exhausted");
      zptr = noise + (size_t)draw * n; philox = 0; off = 0;
    } else { zptr = nullptr; philox = 1; off = (uint64_t)draw * (uint64_t)n_al; }
    ++draw;
    return 0;
  };
  for (int i = Ns - 1; i >= 0; --i) {
    const float tval = (float)i / (float)Ns;
    if (emb_table) run.emb_row = run_corr.emb_row = emb_table + (size_t)i * block;
    else if ((rc = fill_launch(sc.t, tval, B2, s))) return rc;
    if ((rc = unet_forward(net, tl.x2, channels, tl.cond2, channels, sc.t, sc.v, B2, sc.unet_ws, sc.unet_bytes, s, run))) return rc;
    if (mode == MI355_DDIM) {
      if ((rc = ddim_cfg_step_launch(tl.x2, sc.v, w, w_dev, per, tb->sqrt_recip_alphas_cumprod[i], tb->sqrt_recipm1_alphas_cumprod[i],
                                     tb->alphas_cumprod_prev[i], n, s))) return rc;
      continue;
    }
    const float* z = nullptr; int ph = 0; uint64_t off = 0;
    if (i > 0 && (rc = next_noise(z, ph, off))) return rc;
    const float sigma = expf(0.5f * tb->posterior_log_variance_clipped[i]);
    if ((rc = ddpm_cfg_step_launch(tl.x2, sc.v, z, w, w_dev, per, tb->sqrt_recip_alphas_cumprod[i], tb->sqrt_recipm1_alphas_cumprod[i],
                                   tb->posterior_mean_coef1[i], tb->posterior_mean_coef2[i], sigma, ph, opt->seed, off, n, s))) return rc;
    for (int c = 0; c < opt->n_corrector; ++c) {   // at batch B on the first half, as mi355_ddpm_sample runs them
      if ((rc = unet_forward(net, tl.x2, channels, tl.cond2 + n, channels, sc.t, sc.v, batch, sc.unet_ws, sc.unet_bytes, s, run_corr))) return rc;
      const float* z2 = nullptr; int ph2 = 0; uint64_t off2 = 0;
      if ((rc = next_noise(z2, ph2, off2))) return rc;
      const float dt = (opt->tmax - opt->tmin) / (float)Ns;
      if ((rc = corrector_step_launch(tl.x2, sc.v, z2, tb->sqrt_recip_alphas_cumprod[i], tb->sqrt_recipm1_alphas_cumprod[i],
                                      tb->recip_sqrt_m1_alphas_cumprod[i], dt, opt->delta, ph2, opt->seed, off2, n, s))) return rc;
    }
    if (opt->n_corrector > 0) MI355_CHECK_HIP(hipMemcpyAsync(tl.x2 + n, tl.x2, (size_t)n * 4, hipMemcpyDeviceToDevice, s));   // refresh the second half
  }
  if ((rc = clip_launch(tl.x2, -1.f, 1.f, n, s))) return rc;
  MI355_CHECK_HIP(hipMemcpyAsync(x, tl.x2, (size_t)n * 4, hipMemcpyDeviceToDevice, s));
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
  Scratch sd, ss;
  if (int rc = carve(drift, batch, drift_workspace, drift_workspace_bytes, sd)) return rc;
  if (int rc = carve(score, batch, score_workspace, score_workspace_bytes, ss)) return rc;
  hipStream_t s = S(stream);
  const int64_t n = (int64_t)batch * channels * cd.image_size * cd.image_size;
  const int64_t n_al = (n + 3) / 4 * 4;
  // the times the nets see: t_k, or 1 - t_k rounded in fp32 (the notebook's reverse SDE evaluates at `1 - t` of the fp32 tensor)
  std::vector<float> te((size_t)n_steps);
  for (int k = 0; k < n_steps; ++k) te[k] = reverse ? 1.0f - t_grid_host[k] : t_grid_host[k];
  const float *tab_d = nullptr, *tab_s = nullptr;
  if (int rc = make_emb_table(drift, sd, te.data(), n_steps, labels != nullptr, s, &tab_d)) return rc;
  if (int rc = make_emb_table(score, ss, te.data(), n_steps, labels != nullptr, s, &tab_s)) return rc;
  if (tab_d || tab_s) MI355_CHECK_HIP(hipStreamSynchronize(s));   // `te` is a temporary host buffer (once per sample() call)
  UnetRun rd = uniform_t_run(), rs = uniform_t_run();
  rd.labels = rs.labels = labels;
  const size_t blk_d = (size_t)(labels ? drift->num_classes : 1) * drift->emb_total, blk_s = (size_t)(labels ? score->num_classes : 1) * score->emb_total;
  const float ca = reverse ? -1.f : 1.f;
  int rc = 0;
  for (int k = 0; k < n_steps && rc == 0; ++k) {
    const float dt = t_grid_host[k + 1] - t_grid_host[k];
    if (tab_d) rd.emb_row = tab_d + (size_t)k * blk_d;
    else if ((rc = fill_launch(sd.t, te[k], batch, s))) break;
    if (tab_s) rs.emb_row = tab_s + (size_t)k * blk_s;
    else if ((rc = fill_launch(ss.t, te[k], batch, s))) break;
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

// ---- single ops -------------------------------------------------------------------------------------

int mi355_timestep_embedding(const float* t, int batch, int dim, float max_period, float* out, void* stream) {
  MI355_REQUIRE(t && out && batch > 0 && dim > 0, -1, "timestep_embedding: bad argument");
  return timestep_embedding_launch(t, batch, dim, max_period, out, S(stream));
}
int mi355_groupnorm(const float* x, const float* gamma, const float* beta, float* y, int batch, int channels, int hw, int groups,
                    float eps, int silu, void* stream) {
  MI355_REQUIRE(x && gamma && beta && y, -1, "groupnorm: null argument");
  return groupnorm_nchw_launch(x, gamma, beta, y, batch, channels, hw, groups, eps, silu, S(stream));
}
int mi355_euler_step(float* x, const float* v, float dt, int64_t n, void* stream) { return euler_step_launch(x, v, dt, n, S(stream)); }
int mi355_sde_euler_step(float* x, const float* a, const float* b, float ca, float cb, float dt, const float* g, float g_scalar, const float* dW,
                         int use_philox, uint64_t seed, uint64_t offset, float* out, float w, int64_t n, void* stream) {
  MI355_REQUIRE((ca == 1.f || ca == -1.f) && (cb == 1.f || cb == -1.f), -1, "sde_euler_step: ca and cb must be +1 or -1");
  return sde_euler_step_launch(x, a, b, ca, cb, dt, g, g_scalar, dW, use_philox, seed, offset, out, w, n, S(stream));
}
int mi355_ddpm_step(float* x, const float* eps, const float* z, float c_recip, float c_recipm1, float coef1, float coef2,
                    float sigma, int use_philox, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  return ddpm_step_launch(x, eps, z, c_recip, c_recipm1, coef1, coef2, sigma, use_philox, seed, offset, n, S(stream));
}
int mi355_corrector_step(float* x, const float* eps, const float* z, float c_recip, float c_recipm1, float recip_sqrt_m1, float dt,
                         float delta, int use_philox, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  return corrector_step_launch(x, eps, z, c_recip, c_recipm1, recip_sqrt_m1, dt, delta, use_philox, seed, offset, n, S(stream));
}
int mi355_ddim_step(float* x, const float* eps, float c_recip, float c_recipm1, float acp_prev, int64_t n, void* stream) {
  return ddim_step_launch(x, eps, c_recip, c_recipm1, acp_prev, n, S(stream));
}
int mi355_replace_mask(float* x, const float* cond, const float* z, float pad_value, int noisy, float sa, float sb, int use_philox,
                       uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  return replace_mask_launch(x, cond, z, pad_value, noisy, sa, sb, use_philox, seed, offset, n, S(stream));
}
int mi355_clip(float* x, float lo, float hi, int64_t n, void* stream) { return clip_launch(x, lo, hi, n, S(stream)); }
int mi355_guidance_seed(const float* x, const float* eps, const float* cond, float c_recip, float c_recipm1, int mode, float pad_value,
                        int64_t elems_per_sample, float* g_eps, float* g_x, int64_t n, void* stream) {
  return guidance_seed_launch(x, eps, cond, c_recip, c_recipm1, mode, pad_value, elems_per_sample, g_eps, g_x, n, S(stream));
}
int mi355_guidance_update(float* x, const float* g_x, const float* vjp, float scale, int apply, float* update, int64_t n, void* stream) {
  return guidance_update_launch(x, g_x, vjp, scale, apply, update, n, S(stream));
}
int mi355_ema_update(float* target, const float* source, float decay, float one_minus_decay, int64_t n, void* stream) {
  MI355_REQUIRE(target && source, -1, "ema_update: null argument");
  return ema_update_launch(target, source, decay, one_minus_decay, n, S(stream));
}
int mi355_mse_per_sample(const float* a, const float* b, float* out, int batch, int64_t elems_per_sample, void* stream) {
  MI355_REQUIRE(a && b && out, -1, "mse_per_sample: null argument");
  return mse_per_sample_launch(a, b, out, batch, elems_per_sample, S(stream));
}
int mi355_lincomb_per_sample(float* out, const float* x, const float* y, const float* a, const float* b, int batch,
                             int64_t elems_per_sample, void* stream) {
  return lincomb_per_sample_launch(out, x, y, a, b, batch, elems_per_sample, S(stream));
}
int mi355_resize_bilinear(const float* in, float* out, int64_t planes, int h_in, int w_in, int h_out, int w_out, void* stream) {
  return resize_bilinear_launch(in, out, planes, h_in, w_in, h_out, w_out, S(stream));
}
int mi355_paint_patch(const float* images, const int32_t* top, const int32_t* left, int patch_size, float pad_value, int outpaint, float* out,
                      int batch, int channels, int h, int w, void* stream) {
  return paint_patch_launch(images, top, left, patch_size, pad_value, outpaint, out, batch, channels, h, w, S(stream));
}
int mi355_quantize_u8(const float* x, uint8_t* out, int64_t n, void* stream) { return quantize_u8_launch(x, out, n, S(stream)); }
int mi355_to_unit_range(const float* x, float* out, int64_t n, void* stream) { return to_unit_range_launch(x, out, n, S(stream)); }
int mi355_randn(float* out, uint64_t seed, uint64_t offset, int64_t n, void* stream) { return randn_launch(out, seed, offset, n, S(stream)); }

int mi355_rk_combine(float* out, const float* y0, const float* k0, const float* k1, const float* k2, const float* k3, const float* k4,
                     const float* k5, const float* k6, const float* coeff_host, int nk, int64_t n, void* stream) {
  MI355_REQUIRE(coeff_host || nk == 0, -1, "rk_combine: null coefficients");
  const float* k[7] = {k0, k1, k2, k3, k4, k5, k6};
  return rk_combine_launch(out, y0, k, coeff_host, nk, n, S(stream));
}
int mi355_rk_stage(float* out, const float* y0, const float* const k[4], const float* coeff_host, int nk, int64_t n, float* copy_out,
                   uint8_t* u8_out, void* stream) {
  return rk_stage_launch(out, y0, k, coeff_host, nk, n, copy_out, u8_out, S(stream));
}
int mi355_cfg_stage(float* out, const float* y0, const float* const k[4], const float* coeff_host, int nk, int64_t n, float w, const float* w_dev,
                    int64_t elems_per_image, int dup, float* copy_out, uint8_t* u8_out, void* stream) {
  return cfg_stage_launch(out, y0, k, coeff_host, nk, n, w, w_dev, elems_per_image, dup, copy_out, u8_out, S(stream));
}
int mi355_ddpm_cfg_step(float* x, const float* eps, const float* z, float w, const float* w_dev, int64_t elems_per_image, float c_recip, float c_recipm1,
                        float coef1, float coef2, float sigma, int use_philox, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  return ddpm_cfg_step_launch(x, eps, z, w, w_dev, elems_per_image, c_recip, c_recipm1, coef1, coef2, sigma, use_philox, seed, offset, n, S(stream));
}
int mi355_ddim_cfg_step(float* x, const float* eps, float w, const float* w_dev, int64_t elems_per_image, float c_recip, float c_recipm1, float acp_prev,
                        int64_t n, void* stream) {
  return ddim_cfg_step_launch(x, eps, w, w_dev, elems_per_image, c_recip, c_recipm1, acp_prev, n, S(stream));
}
int mi355_rk_sqnorm(const float* a, const float* sub, const float* b, const float* b2, float atol, float rtol, int64_t n, double* out,
                    void* stream) {
  return rk_sqnorm_launch(a, sub, b, b2, atol, rtol, n, out, S(stream));
}
int mi355_rk_interp(float* out, const float* y0, const float* y1, const float* y_mid, const float* f0, const float* f1, float dt, float x,
                    int64_t n, void* stream) {
  return rk_interp_launch(out, y0, y1, y_mid, f0, f1, dt, x, n, S(stream));
}

int64_t mi355_box_probe_workspace_bytes(void) { return box_probe_workspace_bytes(); }
int mi355_box_probe(int reps, void* workspace, int64_t workspace_bytes, void* stream, float* us_per_launch, float* clock_mhz, float* tflop) {
  if (tflop) *tflop = (float)(box_probe_flops() * 1e-12);
  return box_probe_run(reps, workspace, workspace_bytes, S(stream), us_per_launch, clock_mhz);
}
int64_t mi355_box_probe_hbm_workspace_bytes(void) { return box_probe_hbm_workspace_bytes(); }
int mi355_box_probe_hbm(int reps, void* workspace, int64_t workspace_bytes, void* stream, float* us_per_launch, float* gbytes) {
  if (gbytes) *gbytes = (float)(box_probe_hbm_bytes() * 1e-9);
  return box_probe_hbm_run(reps, workspace, workspace_bytes, S(stream), us_per_launch);
}

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
  void* act_dev[2] = {nullptr, nullptr};
  std::vector<char> packed_f; std::vector<float> bias_f;
  if (ex) {
    ex->act_done = 0; ex->skip_done = 0;
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
  ConvRoute route;
  if ((rc = conv_route(d, &route))) {
    if (d.skip_src0) { mi355_set_error("conv2d_ex: this launch cannot carry the fused skip conv (shape, batch or knobs)"); return MI355_ERR_UNSUPPORTED; }
    return rc;
  }
  if ((rc = conv_launch(d, route, s))) return rc;
  if (ex) {
    ex->skip_done = route.skip; ex->act_done = route.act_done;
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

}  // extern "C"
