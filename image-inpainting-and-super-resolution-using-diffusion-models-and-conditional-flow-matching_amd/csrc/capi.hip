// extern "C" boundary of libmi355_sampler.so (see include/mi355_sampler.h): errors, version, handles, forward / vjp / diagnostics and the one-line
// single-op wrappers.  The sampler loops are in samplers.hip, the single-op test harness in test_ops.hip.
#include <cstring>
#include <vector>

#include "capi_internal.h"

static thread_local std::string g_err;
void mi355_set_error(const std::string& msg) { g_err = msg; }

const mi355_debug_config& mi355_default_debug() {
  static const mi355_debug_config d = [] { mi355_debug_config c; mi355_debug_defaults(&c); return c; }();
  return d;
}

extern "C" {

int mi355_version(void) { return 108; }
void mi355_debug_defaults(mi355_debug_config* c) {
  if (!c) return;
  std::memset(c, 0, sizeof(*c));
  c->conv_ws = 3; c->conv_small = 15; c->conv_min_wgs = 512; c->conv_stagger = 0; c->conv_ablate = 0; c->conv_spin_limit = 1 << 22;
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

// mi355_unet_forward_labels and mi355_unet_forward_cached: one body; branch 0 = the whole forward
static int forward_labels_run(const std::string& who, mi355_unet* net, const float* x, int x_channels, const float* cond, int cond_channels, const float* t,
                              float t_host, const int32_t* labels, float* out, int batch, void* workspace, int64_t workspace_bytes, void* stream, int branch) {
  MI355_REQUIRE(net && workspace && batch > 0, -1, who + ": bad argument");
  MI355_REQUIRE(!labels || net->num_classes > 0, -1, who + ": class labels given to a net built without num_classes");
  if (branch) {   // refused here, before the time is staged: nothing is launched
    if (unet_cache_range(net, branch, nullptr, nullptr, nullptr)) { mi355_set_error(who + ": branch: " + mi355_last_error()); return -1; }
    MI355_REQUIRE(!net->cfg.differentiable, -4, who + ": branch: a differentiable plan cannot run a shallow evaluation (the backward pass would see activations of two forwards)");
  }
  UnetRun run;
  run.labels = labels;
  run.reuse_branch = branch;
  if (!t) {   // one host time for the batch: staged as in mi355_unet_forward_t
    const WsLayout l = unet_ws_layout(net, batch);
    MI355_REQUIRE((int64_t)l.total <= workspace_bytes, -2, who + ": workspace too small");
    float* tdev = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + l.emb2);
    if (int rc = fill_launch(tdev, t_host, 1, S(stream))) return rc;
    t = tdev;
    run.t_uniform = 1;
  }
  return unet_forward(net, x, x_channels, cond, cond_channels, t, out, batch, workspace, workspace_bytes, S(stream), run);
}

int mi355_unet_forward_labels(mi355_unet* net, const float* x, int x_channels, const float* cond, int cond_channels, const float* t, float t_host,
                              const int32_t* labels, float* out, int batch, void* workspace, int64_t workspace_bytes, void* stream) {
  return forward_labels_run("unet_forward_labels", net, x, x_channels, cond, cond_channels, t, t_host, labels, out, batch, workspace, workspace_bytes, stream, 0);
}

int mi355_unet_cache_info(const mi355_unet_config* cfg, int branch, int32_t out[8]) {
  MI355_REQUIRE(cfg && out, -1, "unet_cache_info: null argument");
  mi355_unet tmp;
  if (int64_t rc = unet_plan_dry(*cfg, &tmp); rc < 0) return (int)rc;
  for (int i = 0; i < 8; ++i) out[i] = 0;
  out[0] = unet_cache_branches(&tmp);
  if (branch == 0) return 0;
  int lo, hi, tid;
  if (unet_cache_range(&tmp, branch, &lo, &hi, &tid)) { mi355_set_error(std::string("unet_cache_info: branch: ") + mi355_last_error()); return -1; }
  const PlanTensor& t = tmp.tensors[tid];
  out[1] = lo; out[2] = hi; out[3] = tid; out[4] = t.C; out[5] = t.H; out[6] = t.W;
  out[7] = (int32_t)(unet_cache_retained_share(&tmp, branch) * 1e6 + 0.5);
  return 0;
}

int mi355_unet_forward_cached(mi355_unet* net, const float* x, int x_channels, const float* cond, int cond_channels, const float* t, float t_host,
                              const int32_t* labels, float* out, int batch, void* workspace, int64_t workspace_bytes, void* stream, int branch) {
  return forward_labels_run("unet_forward_cached", net, x, x_channels, cond, cond_channels, t, t_host, labels, out, batch, workspace, workspace_bytes, stream,
                            branch);
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
  const WsView v(net, workspace, batch);
  MI355_REQUIRE((int64_t)v.l.total <= workspace_bytes, -2, "read_tensor: workspace too small");
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
  return unpack_nchw_launch(net->cfg.dtype, gradient ? v.grad(tensor) : v.tensor(tensor), batch, t.H * t.W, t.C, out, S(stream));
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
// The predictor-step exports: each fills a PredictorStep for the one launcher (ops.h).
static PredictorStep predictor(int kind, float* x, const float* eps, float c_recip, float c_recipm1, int64_t n) {
  PredictorStep p;
  p.kind = kind; p.x = x; p.eps = eps; p.c_recip = c_recip; p.c_recipm1 = c_recipm1; p.n = n;
  return p;
}
static void with_noise(PredictorStep& p, const float* z, int use_philox, uint64_t seed, uint64_t offset) {
  p.z = z; p.use_philox = use_philox; p.seed = seed; p.offset = offset;
}
static void with_guide(PredictorStep& p, float w, const float* w_dev, int64_t per) { p.guide = {true, w, w_dev}; p.per = per; }
int mi355_ddpm_step(float* x, const float* eps, const float* z, float c_recip, float c_recipm1, float coef1, float coef2,
                    float sigma, int use_philox, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  PredictorStep p = predictor(STEP_ANCESTRAL, x, eps, c_recip, c_recipm1, n);
  p.a = coef1; p.b = coef2; p.sigma = sigma;
  with_noise(p, z, use_philox, seed, offset);
  return predictor_step_launch(p, S(stream));
}
int mi355_corrector_step(float* x, const float* eps, const float* z, float c_recip, float c_recipm1, float recip_sqrt_m1, float dt,
                         float delta, int use_philox, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  return corrector_step_launch(x, eps, z, c_recip, c_recipm1, recip_sqrt_m1, dt, delta, use_philox, seed, offset, n, S(stream));
}
int mi355_ddim_step(float* x, const float* eps, float c_recip, float c_recipm1, float acp_prev, int64_t n, void* stream) {
  PredictorStep p = predictor(STEP_DDIM, x, eps, c_recip, c_recipm1, n);
  p.a = acp_prev;
  return predictor_step_launch(p, S(stream));
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
int mi355_lowres_seed(const float* x, const float* eps, const float* y_low, float c_recip, float c_recipm1, int batch, int channels, int h, int w,
                      int h_low, int w_low, float* resid, float* g_eps, float* g_x, float* loss, void* stream) {
  return lowres_seed_launch(x, eps, y_low, c_recip, c_recipm1, batch, channels, h, w, h_low, w_low, resid, g_eps, g_x, loss, S(stream));
}
int mi355_ema_update(float* target, const float* source, float decay, float one_minus_decay, int64_t n, void* stream) {
  MI355_REQUIRE(target && source, -1, "ema_update: null argument");
  return ema_update_launch(target, source, decay, one_minus_decay, n, S(stream));
}
int mi355_mse_per_sample(const float* a, const float* b, float* out, int batch, int64_t elems_per_sample, void* stream) {
  MI355_REQUIRE(a && b && out, -1, "mse_per_sample: null argument");
  return mse_per_sample_launch(a, b, out, batch, elems_per_sample, S(stream));
}
int mi355_feature_drift(const void* cur, void* prev, int dtype, int batch, int64_t elems_per_image, float* out, void* stream) {
  MI355_REQUIRE(dtype == MI355_F32 || dtype == MI355_BF16 || dtype == MI355_BF16X2 || dtype == MI355_F16, -1,
                "feature_drift: dtype must be MI355_F32, MI355_BF16, MI355_BF16X2 or MI355_F16");
  return feature_drift_launch(dtype == MI355_F16 ? DT_F16 : (dtype == MI355_F32 ? DT_F32 : DT_BF16), cur, prev, batch, elems_per_image, out, S(stream));
}
int mi355_image_metrics(const float* x, const float* ref, float* out, int batch, int channels, int h, int w, float data_range,
                        const float* taps_host, int win, float cov_norm, float k1, float k2, void* stream) {
  MI355_REQUIRE(x, -1, "image_metrics: x is null");
  MI355_REQUIRE(ref, -1, "image_metrics: ref is null");
  MI355_REQUIRE(out, -1, "image_metrics: out is null");
  return image_metrics_launch(x, ref, out, batch, channels, h, w, data_range, taps_host, win, cov_norm, k1, k2, S(stream));
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
  PredictorStep p = predictor(STEP_ANCESTRAL, x, eps, c_recip, c_recipm1, n);
  p.a = coef1; p.b = coef2; p.sigma = sigma;
  with_noise(p, z, use_philox, seed, offset);
  with_guide(p, w, w_dev, elems_per_image);
  return predictor_step_launch(p, S(stream));
}
int mi355_ddim_cfg_step(float* x, const float* eps, float w, const float* w_dev, int64_t elems_per_image, float c_recip, float c_recipm1, float acp_prev,
                        int64_t n, void* stream) {
  PredictorStep p = predictor(STEP_DDIM, x, eps, c_recip, c_recipm1, n);
  p.a = acp_prev;
  with_guide(p, w, w_dev, elems_per_image);
  return predictor_step_launch(p, S(stream));
}
int mi355_ddim_eta_step(float* x, const float* eps, const float* z, float c_recip, float c_recipm1, float acp_prev, float sigma, int use_philox,
                        uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  PredictorStep p = predictor(STEP_DDIM_ETA, x, eps, c_recip, c_recipm1, n);
  p.a = acp_prev; p.sigma = sigma;
  with_noise(p, z, use_philox, seed, offset);
  return predictor_step_launch(p, S(stream));
}
int mi355_ddim_eta_cfg_step(float* x, const float* eps, const float* z, float w, const float* w_dev, int64_t elems_per_image, float c_recip,
                            float c_recipm1, float acp_prev, float sigma, int use_philox, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  PredictorStep p = predictor(STEP_DDIM_ETA, x, eps, c_recip, c_recipm1, n);
  p.a = acp_prev; p.sigma = sigma;
  with_noise(p, z, use_philox, seed, offset);
  with_guide(p, w, w_dev, elems_per_image);
  return predictor_step_launch(p, S(stream));
}
int mi355_renoise_step(float* x, const float* z, float a, float b, int use_philox, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  return renoise_step_launch(x, z, a, b, use_philox, seed, offset, n, S(stream));
}
int mi355_nullspace_step(const mi355_nullspace_op* op, int form, int pred_kind, float* x, const float* out, int64_t out_stride, const float* y,
                         const float* z, int batch, int channels, int h, int w, float c_recip, float c_recipm1, float sa, float sb, float a, float b,
                         float lam, float sigma, int use_philox, uint64_t seed, uint64_t offset, void* stream) {
  NullspaceStep p;
  p.op = op; p.form = form; p.pred = pred_kind; p.x = x; p.out = out; p.out_stride = out_stride; p.y = y; p.z = z;
  p.batch = batch; p.channels = channels; p.h = h; p.w = w;
  p.c_recip = c_recip; p.c_recipm1 = c_recipm1; p.sa = sa; p.sb = sb; p.a = a; p.b = b; p.lam = lam; p.sigma = sigma;
  p.use_philox = use_philox; p.seed = seed; p.offset = offset;
  return nullspace_step_launch(p, S(stream));
}
int mi355_block_mean(const float* in, float* out, int64_t planes, int h, int w, int h_low, int w_low, void* stream) {
  return block_mean_launch(in, out, planes, h, w, h_low, w_low, S(stream));
}
int mi355_dpmpp_step(float* x, const float* eps, float* hist, float c_recip, float c_recipm1, float cx, float c0, float c1, int64_t n, void* stream) {
  PredictorStep p = predictor(STEP_DPMPP, x, eps, c_recip, c_recipm1, n);
  p.hist = hist; p.a = cx; p.b = c0; p.c = c1;
  return predictor_step_launch(p, S(stream));
}
int mi355_dpmpp_cfg_step(float* x, const float* eps, float* hist, float w, const float* w_dev, int64_t elems_per_image, float c_recip, float c_recipm1,
                         float cx, float c0, float c1, int64_t n, void* stream) {
  PredictorStep p = predictor(STEP_DPMPP, x, eps, c_recip, c_recipm1, n);
  p.hist = hist; p.a = cx; p.b = c0; p.c = c1;
  with_guide(p, w, w_dev, elems_per_image);
  return predictor_step_launch(p, S(stream));
}
int mi355_x0_shape_stats(const float* x, const float* eps, float w, const float* w_dev, int guided, float c_recip, float c_recipm1,
                         const mi355_x0_shaping* shaping, float* shape, float* detail, int batch, int64_t elems_per_image, void* stream) {
  return x0_shape_stats_launch(x, eps, StepGuide{guided != 0, w, w_dev}, c_recip, c_recipm1, shaping, shape, detail, batch, elems_per_image, S(stream));
}
// One shaped (or, shape == null, unshaped) predictor step chosen by number: 0 ancestral (a, b = coef1, coef2), 1 DDIM (a = acp_prev), 2 DDIM(eta)
// (a = acp_prev), 3 DPM-Solver++ (a, b, c = cx, c0, c1); the numbers are the STEP_* kinds.
int mi355_x0_shaped_step(int kind, float* x, const float* eps, const float* z, float* hist, int guided, float w, const float* w_dev,
                         int64_t elems_per_image, float c_recip, float c_recipm1, float a, float b, float c, float sigma, int use_philox, uint64_t seed,
                         uint64_t offset, const float* shape, int64_t n, void* stream) {
  const int64_t per = elems_per_image;
  MI355_REQUIRE(kind >= 0 && kind <= 3, -1, "x0_shaped_step: kind must be 0 (ancestral), 1 (DDIM), 2 (DDIM(eta)) or 3 (DPM-Solver++)");
  MI355_REQUIRE(per > 0 && n % per == 0, -1, "x0_shaped_step: n must be whole images of elems_per_image elements");
  PredictorStep p = predictor(kind, x, eps, c_recip, c_recipm1, n);
  p.hist = hist; p.a = a; p.b = b; p.c = c; p.sigma = sigma; p.shape = shape; p.per = per;
  with_noise(p, z, use_philox, seed, offset);
  if (guided) with_guide(p, w, w_dev, per);
  return predictor_step_launch(p, S(stream));
}
// The steps above on a network output wider than the state (a learned-variance net's [B, 2C, H, W]): eps of image b at eps + b * eps_stride.  kind 0..3
// as mi355_x0_shaped_step; 4: the Langevin corrector (a, b, c = recip_sqrt_m1, dt, delta; never guided).
int mi355_strided_step(int kind, float* x, const float* eps, int64_t eps_stride, const float* z, float* hist, int guided, float w, const float* w_dev,
                       int64_t elems_per_image, float c_recip, float c_recipm1, float a, float b, float c, float sigma, int use_philox, uint64_t seed,
                       uint64_t offset, int64_t n, void* stream) {
  const int64_t per = elems_per_image;
  MI355_REQUIRE(kind >= 0 && kind <= 4, -1, "strided_step: kind must be 0 (ancestral), 1 (DDIM), 2 (DDIM(eta)), 3 (DPM-Solver++) or 4 (corrector)");
  MI355_REQUIRE(per > 0 && n % per == 0, -1, "strided_step: n must be whole images of elems_per_image elements");
  MI355_REQUIRE(eps_stride >= per, -1, "strided_step: eps_stride must be >= elems_per_image");
  if (kind == 4) {
    MI355_REQUIRE(!guided, -1, "strided_step: the corrector has no guided form");
    MI355_REQUIRE(n <= 0 || (x && eps), -1, "strided_step: null argument");
    return corrector_step_launch(x, eps, z, c_recip, c_recipm1, a, b, c, use_philox, seed, offset, n, S(stream), per, eps_stride);
  }
  PredictorStep p = predictor(kind, x, eps, c_recip, c_recipm1, n);
  p.hist = hist; p.a = a; p.b = b; p.c = c; p.sigma = sigma; p.per = per; p.eps_stride = eps_stride;
  with_noise(p, z, use_philox, seed, offset);
  if (guided) with_guide(p, w, w_dev, per);
  return predictor_step_launch(p, S(stream));
}
// The ancestral step of a learned-variance net: out [batch (guided: 2 batch), 2C, H, W] is the network output, eps in channels [0, C), v in [C, 2C).
int mi355_ddpm_lv_step(float* x, const float* out, const float* z, float w, const float* w_dev, int guided, int64_t elems_per_image, float c_recip,
                       float c_recipm1, float coef1, float coef2, float min_log, float max_log, int use_philox, uint64_t seed, uint64_t offset, int batch,
                       void* stream) {
  MI355_REQUIRE(elems_per_image > 0, -1, "ddpm_lv_step: elems_per_image must be > 0");
  MI355_REQUIRE(batch >= 0, -1, "ddpm_lv_step: batch must be >= 0");
  PredictorStep p = predictor(STEP_ANCESTRAL_LV, x, out, c_recip, c_recipm1, (int64_t)batch * elems_per_image);
  p.a = coef1; p.b = coef2; p.min_log = min_log; p.max_log = max_log; p.per = elems_per_image; p.eps_stride = 2 * elems_per_image;
  with_noise(p, z, use_philox, seed, offset);
  if (guided) with_guide(p, w, w_dev, elems_per_image);
  return predictor_step_launch(p, S(stream));
}
// The variational bound's launches as ops (vlb.hip, steps.hip): the noising q(x_k | x_0), one step's terms, the prior term and the total.
int mi355_q_sample(float* out, const float* x0, const float* z, float a, float b, int use_philox, uint64_t seed, uint64_t offset, int64_t n, void* stream) {
  return q_sample_launch(out, x0, z, a, b, use_philox, seed, offset, n, S(stream));
}
int mi355_vlb_terms(const float* x0, const float* x_k, const float* out, int64_t out_stride, const float* z, int use_philox, uint64_t seed, uint64_t offset,
                    float c_recip, float c_recipm1, float coef1, float coef2, float true_log, float model_log, float min_log, float max_log, int k_is_zero,
                    int learned, int cdf, int clip_denoised, float* dst, int64_t dst_stride, int batch, int64_t elems_per_image, void* stream) {
  VlbStep st;
  st.c_recip = c_recip; st.c_recipm1 = c_recipm1; st.coef1 = coef1; st.coef2 = coef2;
  st.true_log = true_log; st.model_log = model_log; st.min_log = min_log; st.max_log = max_log;
  st.k_is_zero = k_is_zero; st.learned = learned; st.cdf = cdf; st.clip = clip_denoised;
  return vlb_terms_launch(x0, x_k, out, out_stride, z, use_philox, seed, offset, st, dst, dst_stride, batch, elems_per_image, S(stream));
}
// The steps, the statistics and the bound's terms of a net whose output is x0 or v (mi355_ddpm_prediction): the ops above with the prediction kind and
// sa, sb = sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod of the step (read by kind 2 alone).
// mi355_pred_step - kind 0..3: the predictor steps of mi355_x0_shaped_step; 4: the Langevin corrector (a, b, c = recip_sqrt_m1, dt, delta; never guided,
// never shaped); 5: the learned-variance ancestral step (a, b = coef1, coef2; out_stride >= 2 * elems_per_image).  out_stride 0: contiguous.
int mi355_pred_step(int kind, int pred_kind, float* x, const float* out, int64_t out_stride, const float* z, float* hist, int guided, float w,
                    const float* w_dev, int64_t elems_per_image, float c_recip, float c_recipm1, float sa, float sb, float a, float b, float c, float sigma,
                    float min_log, float max_log, int use_philox, uint64_t seed, uint64_t offset, const float* shape, int64_t n, void* stream) {
  const int64_t per = elems_per_image;
  MI355_REQUIRE(kind >= 0 && kind <= 5, -1,
                "pred_step: kind must be 0 (ancestral), 1 (DDIM), 2 (DDIM(eta)), 3 (DPM-Solver++), 4 (corrector) or 5 (learned-variance ancestral)");
  MI355_REQUIRE(pred_kind >= PRED_EPS && pred_kind <= PRED_V, -1, "pred_step: pred_kind must be 0 (eps), 1 (x0) or 2 (v)");
  MI355_REQUIRE(per > 0 && n % per == 0, -1, "pred_step: n must be whole images of elems_per_image elements");
  MI355_REQUIRE(out_stride == 0 || out_stride >= per, -1, "pred_step: out_stride must be 0 (contiguous) or >= elems_per_image");
  if (kind == 4) {
    MI355_REQUIRE(!guided, -1, "pred_step: the corrector has no guided form");
    MI355_REQUIRE(!shape, -1, "pred_step: the corrector keeps the static clip (shape must be NULL)");
    MI355_REQUIRE(n <= 0 || (x && out), -1, "pred_step: null argument");
    return corrector_step_launch(x, out, z, c_recip, c_recipm1, a, b, c, use_philox, seed, offset, n, S(stream), per, out_stride, pred_kind, sa, sb);
  }
  PredictorStep p = predictor(kind == 5 ? STEP_ANCESTRAL_LV : kind, x, out, c_recip, c_recipm1, n);
  p.hist = hist; p.a = a; p.b = b; p.c = c; p.sigma = sigma; p.shape = shape; p.per = per; p.eps_stride = out_stride;
  p.min_log = min_log; p.max_log = max_log; p.pred = pred_kind; p.sa = sa; p.sb = sb;
  with_noise(p, z, use_philox, seed, offset);
  if (guided) with_guide(p, w, w_dev, per);
  return predictor_step_launch(p, S(stream));
}
int mi355_pred_shape_stats(int pred_kind, const float* x, const float* out, float w, const float* w_dev, int guided, float c_recip, float c_recipm1,
                           float sa, float sb, const mi355_x0_shaping* shaping, float* shape, float* detail, int batch, int64_t elems_per_image,
                           void* stream) {
  return x0_shape_stats_launch(x, out, StepGuide{guided != 0, w, w_dev}, c_recip, c_recipm1, shaping, shape, detail, batch, elems_per_image, S(stream),
                               pred_kind, sa, sb);
}
int mi355_vlb_terms_pred(const float* x0, const float* x_k, const float* out, int64_t out_stride, const float* z, int use_philox, uint64_t seed,
                         uint64_t offset, float c_recip, float c_recipm1, float coef1, float coef2, float true_log, float model_log, float min_log,
                         float max_log, int k_is_zero, int learned, int cdf, int clip_denoised, int pred_kind, float sa, float sb, float* dst,
                         int64_t dst_stride, int batch, int64_t elems_per_image, void* stream) {
  VlbStep st;
  st.c_recip = c_recip; st.c_recipm1 = c_recipm1; st.coef1 = coef1; st.coef2 = coef2;
  st.true_log = true_log; st.model_log = model_log; st.min_log = min_log; st.max_log = max_log;
  st.k_is_zero = k_is_zero; st.learned = learned; st.cdf = cdf; st.clip = clip_denoised;
  st.pred = pred_kind; st.sa = sa; st.sb = sb;
  return vlb_terms_launch(x0, x_k, out, out_stride, z, use_philox, seed, offset, st, dst, dst_stride, batch, elems_per_image, S(stream));
}
int mi355_vlb_prior(const float* x0, float sqrt_acp_last, float sqrt_one_minus_acp_last, const float* terms, int64_t terms_stride, int n_steps,
                    float* summary, int batch, int64_t elems_per_image, void* stream) {
  return vlb_prior_launch(x0, sqrt_acp_last, sqrt_one_minus_acp_last, terms, terms_stride, n_steps, summary, batch, elems_per_image, S(stream));
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

}  // extern "C"
