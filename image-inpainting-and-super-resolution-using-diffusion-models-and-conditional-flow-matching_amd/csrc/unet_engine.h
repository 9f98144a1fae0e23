// U-Net layer plan + executor (host C++).  See unet_engine.hip.
#pragma once
#include <string>
#include <variant>
#include <vector>

#include "../../include/mi355_sampler.h"
#include <atomic>
#include <memory>
#include <mutex>

#include "ops.h"

struct ParamInfo {
  std::string name;
  std::vector<int64_t> shape;
  int64_t numel() const { int64_t n = 1; for (auto s : shape) n *= s; return n; }
};

// Parameter inventory in reference state_dict order (UNetModel.__init__, unet.py:564-706).
int unet_enumerate_params(const mi355_unet_config& cfg, std::vector<ParamInfo>& out);

struct PlanTensor {
  int C, H, W; bool f32; size_t offset_per_image;   // element type T unless f32
  // fused GroupNorm statistics (common.h GnPartial): set when a GroupNorm site that takes its (a, b) from partial sums reads this
  // tensor; the producing conv fills stats[N][slots][C/4][2] at stats_off_per_image * N floats into the statistics arena
  int stats_cap = 0; size_t stats_off_per_image = 0;
};
// PlanTensor::stats_cap of a tensor of HW pixels: >= the slots of every kernel variant (at most one slot per 32 pixels)
inline int gn_stats_cap(int HW) { return 4 * ((HW + 63) / 64) + 8; }

enum OpKind { OP_GN = 0, OP_CONV = 1, OP_ATTN = 2, OP_RESAMPLE = 3, OP_POOLAFF = 4, OP_ATTN_FUSED = 5 };

struct PlanOp {
  int kind;
  // common
  int src0 = -1, src1 = -1, dst = -1;
  // GN
  size_t gamma_off = 0, beta_off = 0; int film_emb_off = -1;
  int fin_ok = 0;   // this site's groups are whole channel quads of each source: (a, b) may come from the producers' partial sums
  int gn_site = -1; // differentiable plans: OP_GN = its site; OP_CONV / OP_POOLAFF with a prologue = the site whose (a, b) they apply
  size_t wT_off = 0; int cin_pad = 0;   // differentiable plans: data-gradient weights (conv_pack_weights_dgrad) and their output channels
  // conv
  int mode = 0, ks = 3, Cout = 0; size_t w_off = 0, bias_off = 0;
  int use_pro = 0, pro_silu = 0; int emb_off = -1; int res = -1, res_mode = 0; int out_mode = 0;
  // attention
  int heads = 0, ch = 0;
  // small levels: a ResBlock's 1x1 skip_connection op names the second conv that can carry it (carrier), and that conv names the skip op
  // (skip_op) and holds the fused weight image / summed bias (conv_pack_weights_skip); decided per launch (conv_route)
  int carrier = -1, skip_op = -1; size_t wf_off = 0, bf_off = 0;
  // prologue-free conv over a nearest-x2 up-sample (Upsample.conv): a second weight image, the filter collapsed to four 2x2 phase filters
  // (conv_pack_weights_up2), for the ping-pong kernel's phase form; both images are kept, the route decides per launch
  int has_wu = 0; size_t wu_off = 0;
};
// PlanOp::cin_pad of a conv over sources of C0 (+ C1) channels: NHWC conv outputs come in whole 32-channel tiles
inline int conv_dgrad_cin_pad(int C0, int C1) { return (C0 + C1 + 31) / 32 * 32; }

struct mi355_unet {
  mi355_unet_config cfg;
  mi355_debug_config knobs;        // diagnostic switches, copied at creation (cfg.debug is not kept)
  // error word of the handle's launches: pinned host memory the kernels write through (mi355_unet_status); dev = its device address
  uint32_t* err_host = nullptr; uint32_t* err_dev = nullptr;
  ~mi355_unet();
  std::vector<ParamInfo> params;
  std::vector<PlanTensor> tensors;
  std::vector<PlanOp> ops;
  char* dev_weights = nullptr;
  int64_t dev_weights_bytes = 0;
  // fp32 side tables in the weight blob
  size_t te_w0 = 0, te_b0 = 0, te_w2 = 0, te_b2 = 0, emb_w = 0, emb_b = 0;
  int emb_total = 0;   // concatenated emb_layers output channels of all ResBlocks
  int num_classes = 0; size_t label_w = 0;   // class-conditional nets: label_emb.weight, fp32 [num_classes][4 mc]
  int in_pad = 0;      // first conv's padded input channels
  int max_gn_c = 0;
  size_t act_elems_per_image = 0;  // activation arena (elements of T) per image
  size_t stats_floats_per_image = 0;   // partial GroupNorm statistics arena (fp32) per image
  // differentiable plans (reconstruction guidance): per-site (a, b, mean, rstd) kept by the forward, and the backward's scratch sizes
  std::vector<int> site_C; std::vector<size_t> site_off;   // site k: a[C] | b[C] | mean[32] | rstd[32] floats per image at site_off[k]
  size_t site_floats_per_image = 0;
  size_t bwd_du_elems = 0, bwd_tmp_elems = 0, bwd_z_elems = 0, bwd_ld_floats = 0;   // per image
  int in_tensor = -1, out_channels = 0;
  // stats per image
  double conv_flops = 0, attn_flops = 0, act_bytes = 0, weight_bytes = 0;
  // Feature reuse across sampler steps (DeepCache).  The blocks of UNetModel as the plan lays them out: first plan op of input_blocks[i] and of
  // output_blocks[i] (n of each), the tensor id of h entering output_blocks[i] (before its concat), and conv_flops + attn_flops planned before
  // each of those ops.  Set by the plan walk, never changed afterwards (unet_cache_range reads them).
  std::vector<int> in_block_op, out_block_op, out_block_h;
  std::vector<double> in_block_flops, out_block_flops;
  int wsplit = 0;         // MI355_BF16X2: conv / qkv weights packed as hi | lo bf16 halves along K (ConvDesc::wsplit)
  int64_t launches = 0;   // device launches of one forward as planned (an upper bound: a GroupNorm pass a conv epilogue absorbed is not launched)
  mutable int64_t last_launches = 0;   // what the most recent forward really launched (0 before the first)
  // what the most recent forward left in each activation tensor (diagnostics: mi355_unet_read_tensor): 0 = the tensor as the reference
  // defines it, 1 = never written (its only reader, a GroupNorm site, was fused into the producing conv's epilogue), 2 = overwritten in
  // place by silu?(GroupNorm(.)) (16x16 level).  Sized at build.  The record is PER HANDLE (of whichever forward wrote it last, on any workspace or
  // batch size): relaxed atomic bytes, so concurrent forwards of one handle from several threads are race-free and only blur the diagnostic.
  mutable std::unique_ptr<std::atomic<char>[]> tensor_state;
  size_t tensor_state_n = 0;
  // knobs.sampler_graph: the flow-matching Euler loop of mi355_cfm_euler_sample as instantiated hipGraphs, one per (workspace, batch, schedule,
  // condition) the handle has been driven with (a few entries, least recently used replaced).  Guarded by graph_mu: the cache is the one piece of
  // handle state a sampler call changes.
  struct SamplerGraph { uint64_t key[8] = {0}; hipGraphExec_t exec = nullptr; uint64_t stamp = 0; int64_t launches = 0; };
  mutable std::mutex graph_mu;
  mutable std::vector<SamplerGraph> graphs;
  mutable hipStream_t capture_stream = nullptr;
  mutable uint64_t graph_clock = 0;
};

// Per-call options of unet_forward.  They are arguments, not handle state: a handle is immutable after unet_build, so one
// handle may be driven from several host threads / streams (each with its own workspace).
struct UnetRun {
  int t_uniform = 0;   // sampler loops: t[0] holds for the whole batch (one embedding row, stride-0 broadcast)
  const float* emb_row = nullptr;   // sampler loops: this step's row of a precomputed table of all emb_layers outputs
                                    // (unet_embedding_table): the four time-embedding launches are skipped
  // sampler loops (flow-matching Euler): x += euler_dt * (network output) in the last conv's epilogue where that conv runs on the streaming kernel
  // (the output tensor is then not written); else unet_forward adds the step launch itself.  euler_x may be the network input x.
  float* euler_x = nullptr; float euler_dt = 0.f;
  // class-conditional nets: device int32[B] labels (emb = time_embed(.) + label_emb(labels)): every image gets its own embedding row.  With
  // emb_row set, emb_row is this step's block of a (step, class) table [num_classes][emb_total] and the images' rows are gathered from it
  // (one launch); without, the rows are computed from t and the labels (unet_embedding_rows_labels, the usual four launches)
  const int32_t* labels = nullptr;
  // Feature reuse (DeepCache): 0 = the whole forward.  k in 1..n-1 (n = the net's input / output blocks) = a SHALLOW evaluation of branch k:
  // input_blocks[0..k-1] on this call's x, then output_blocks[n-k..n-1] and out on the feature h that the most recent WHOLE forward on this
  // workspace at this batch left in front of output_blocks[n-k].  The forward is resolved exactly as with 0; the plan ops of unet_cache_range
  // are then not issued.  The caller's contract (not checkable here): that previous forward was a whole one.
  int reuse_branch = 0;
  // optional per-op profiling (mi355_unet_profile)
  std::vector<mi355_op_profile>* prof = nullptr;
  std::vector<hipEvent_t>* prof_events = nullptr;
};

int unet_build(const mi355_unet_config& cfg, const float* const* params_host, int n_params, void* dev_weights,
               int64_t dev_weights_bytes, hipStream_t stream, mi355_unet** out);
int64_t unet_weight_bytes(const mi355_unet_config& cfg);
int unet_status(const mi355_unet* net, int clear);   // 0 or MI355_ERR_TIMEOUT (+ message)
int64_t unet_workspace_bytes(const mi355_unet* net, int batch);
struct WsLayout { size_t temb, emb1, emb2, embp, gna, gnb, stats, sites, arena, grads, du, tmp, z, dy, ld, total; };
WsLayout unet_ws_layout(const mi355_unet* net, int B);
// One call's view of a workspace: the regions of unet_ws_layout at batch B as pointers (forward, backward and mi355_unet_read_tensor).
struct WsView {
  const mi355_unet* net; char* ws; WsLayout l; size_t B, esz;
  WsView(const mi355_unet* n, void* workspace, int batch)
      : net(n), ws(reinterpret_cast<char*>(workspace)), l(unet_ws_layout(n, batch)), B((size_t)batch), esz(n->cfg.dtype == 0 ? 4 : 2) {}
  float* f32(size_t off) const { return reinterpret_cast<float*>(ws + off); }
  void* at(size_t off) const { return ws + off; }
  void* tensor(int id) const { return id < 0 ? nullptr : ws + l.arena + net->tensors[id].offset_per_image * B * esz; }   // activation (NHWC)
  void* grad(int id) const { return id < 0 ? nullptr : ws + l.grads + net->tensors[id].offset_per_image * B * esz; }     // its gradient (differentiable plans)
  float* stats(int id) const { return f32(l.stats) + net->tensors[id].stats_off_per_image * B; }   // partial GroupNorm sums its producer leaves
  // differentiable plans: GroupNorm site k's own a[B][C] | b[B][C] | mean[B][32] | rstd[B][32]
  struct Site { float *a, *b, *mean, *rstd; };
  Site site(int k) const {
    float* sp = f32(l.sites) + net->site_off[k] * B;
    const size_t BC = B * (size_t)net->site_C[k];
    return {sp, sp + BC, sp + 2 * BC, sp + 2 * BC + B * 32};
  }
};
// (d out / d x)^T grad_out of the last unet_forward on this workspace (differentiable plans only; unet_backward.hip)
int unet_backward(const mi355_unet* net, const float* grad_out, float* grad_x, int Cx, int batch, void* workspace, int64_t workspace_bytes,
                  hipStream_t stream);
// All emb_layers outputs (UNetModel.time_embed + every ResBlock's emb_layers, unet.py:564-569,293-299) for n step times at once:
// table [n][emb_total] fp32; scratch = n * 9 * model_channels floats.  The sampler loops know every step time in advance.
int unet_embedding_table(const mi355_unet* net, const float* t_dev, int n, float* table, float* scratch, hipStream_t stream);
// Class-conditional form: h = time_embed(timestep_embedding(t)) (before the SiLU) for n_t times, then rows r < R of
// table = emb_layers(silu(h[r / h_div] + label_emb[lab(r)])), lab(r) = labels ? labels[r] : r % num_classes.  scratch = n_t * 9 * mc floats.
int unet_embedding_rows_labels(const mi355_unet* net, const float* t_dev, int n_t, const int32_t* labels, int R, int h_div, float* table,
                               float* scratch, hipStream_t stream);
int unet_forward(const mi355_unet* net, const float* x, int Cx, const float* cond, int Cc, const float* t, float* out, int batch,
                 void* workspace, int64_t workspace_bytes, hipStream_t stream, const UnetRun& run = UnetRun());

// ---- a forward, resolved ---------------------------------------------------------------------------------------------------------------
// unet_forward = unet_resolve, then issue.  unet_resolve is pure host code: no HIP call, no handle state touched; it walks the plan once and
// says what each plan op becomes in THIS forward (batch, knobs, run options) with the descriptor it is launched with.  The result is a local
// value of the call: nothing of it is kept on the handle.
struct GnAbsorbed {};    // GroupNorm site applied by its producers' epilogues: nothing launched
struct ConvCarried {};   // 1x1 skip conv riding in its ResBlock's second conv (the next step): nothing launched, its tensor never written
struct ConvStep { ConvDesc c; ConvRoute rt; };
struct PoolAffStep { int dtype; const void* in; const float* a; const float* b; int silu; void* out; int N, H, W, C; };   // affine_pool_launch's arguments
struct ResampleStep { int dtype; const void* in; void* out; int N, H, W, C, mode; };                                      // resample_launch's
// GnFinDesc: (a, b) finalized from the producers' partial sums; GnDesc: the statistics (/ apply) pass
using ForwardStep = std::variant<GnAbsorbed, GnFinDesc, GnDesc, ConvStep, ConvCarried, AttnDesc, AttnFusedDesc, PoolAffStep, ResampleStep>;
enum EmbPath { EMB_ROW = 0, EMB_GATHER, EMB_LABELS, EMB_TIME };   // the caller's row as it is | rows gathered by label | computed from t and labels | from t
struct ResolvedForward {
  int emb = EMB_TIME, Be = 0, estride = 0; const float* embp = nullptr;   // embedding path, its rows (Be times) and their stride for the consumers
  bool pack = true;                 // false: the first conv reads the caller's NCHW tensors itself (no pack_nhwc launch)
  std::vector<ForwardStep> steps;   // one per plan op, in plan order
  bool euler_in_conv = false;       // the last conv's epilogue applies UnetRun's Euler update
  // UnetRun::reuse_branch: steps [skip_lo, skip_hi) are resolved (what they settle for later steps stands) but not issued; empty for a whole forward
  size_t skip_lo = 0, skip_hi = 0;
  bool issued(size_t i) const { return i < skip_lo || i >= skip_hi; }
};
int unet_resolve(const WsView& v, const float* x, int Cx, const float* cond, int Cc, float* out, const UnetRun& run, ResolvedForward* f);
inline bool unet_step_launches(const ForwardStep& s) { return !std::holds_alternative<GnAbsorbed>(s) && !std::holds_alternative<ConvCarried>(s); }
// Branch k of the feature cache: the plan ops [*lo, *hi) a shallow evaluation does not issue (input_blocks[k] .. the producer of the cached
// feature) and the cached feature's tensor id.  n - 1 branches (unet_cache_branches).  k outside 1..n-1: MI355_ERR_ARG with a message.
int unet_cache_branches(const mi355_unet* net);
int unet_cache_range(const mi355_unet* net, int k, int* lo, int* hi, int* tensor);
double unet_cache_retained_share(const mi355_unet* net, int k);   // of conv_flops + attn_flops, for a valid k
int64_t unet_launch_count(const ResolvedForward& f);   // launches the issue pass makes (the sampler's Euler step not counted)
// the plan alone, no host parameters and no weight image: the bytes that image would take, or < 0
int64_t unet_plan_dry(const mi355_unet_config& cfg, mi355_unet* net);
