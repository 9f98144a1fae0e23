// Host-only record of what the sampler entry points of libmi355_sampler.so answer before they touch a device: every mi355_*_workspace_bytes
// value, and for every sampler entry point (the tiled ones and the predictor-step exports included) the return code and mi355_last_error() text of
// a list of calls with ONE fault each.  Nets are planned with unet_plan_dry and driven with made-up pointers, as tools/resolve_steps.hip does; nothing is launched and no
// device is needed.  Every call the program makes must be refused before its first HIP call, in words that name the faulted argument: a case that
// returns 0 or -3 (a HIP error), or that is refused for another reason, fails the program.  No call is made that the host checks would accept, and
// the program must not be run where a device is present (it refuses to start there): an accepted call would launch on made-up addresses.
// Build it with the host code under a sanitizer (make -C <package>/csrc sampler_refusals) and run it: it must exit 0 with no report.  Two builds of
// the library whose host code checks the same things in the same words print the same bytes: keep the output of the build before a change of the
// sampler host code and compare.  It is a program of its own: never load it into Python.
#include <unistd.h>

#include <cstdio>
#include <cstring>
#include <string>

#include "../image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd/csrc/unet_engine.h"

namespace {

mi355_unet_config cifar() {
  mi355_unet_config c{};
  c.image_size = 32; c.in_channels = 3; c.model_channels = 128; c.out_channels = 3; c.num_res_blocks = 2;
  c.n_attention_ds = 1; c.attention_ds[0] = 2;
  c.n_channel_mult = 4; const int m[4] = {1, 2, 2, 2}; memcpy(c.channel_mult, m, sizeof m);
  c.conv_resample = 1; c.num_heads = 4; c.num_head_channels = 64; c.num_heads_upsample = -1;
  c.dtype = MI355_BF16;
  return c;
}
// class-conditional and amortized (a 2C-input net): the plan the guided entry points accept
mi355_unet_config classcond() {
  mi355_unet_config c = cifar();
  c.in_channels = 6; c.num_classes = 10;
  return c;
}

template <class T> T* fake(int k) { return reinterpret_cast<T*>(uintptr_t(k) << 40); }   // made-up addresses, never dereferenced
constexpr int K = 4;          // DDPM steps of the host tables

// Every argument of every entry point, at values the plan accepts; a case builds a fresh one and changes one thing.
struct Args {
  mi355_unet* net; mi355_unet* score; bool classy;
  float* x = fake<float>(3); int channels = 3; const float* cond = nullptr; int cond_channels = 0; const int32_t* labels = nullptr;
  float none_value = -2.f; int null_label = 9; float w = 2.f; const float* w_dev = nullptr; int guided = 0;
  int batch; void* ws = fake<void>(2); int64_t ws_bytes = int64_t(1) << 50; void* ws2 = fake<void>(6);
  // flows: a span of three steps, explicit midpoint, AB2 weights for it
  float t_span[4] = {0.f, 0.25f, 0.5f, 1.f}; const float* ts = t_span; int n_t = 4;
  int stages = 2; float a[4] = {0.f, 0.f, 0.5f, 0.f}, b[2] = {0.f, 1.f}, c[2] = {0.f, 0.5f};
  const float* ap = a; const float* bp = b; const float* cp = c;
  int order = 2; float wab[6] = {0.f, 0.f, 0.375f, -0.125f, 0.75f, -0.25f}; const float* wp = wab;
  // recon: painting with coupled replacement
  const float* y = fake<float>(7); int mode = 0, h_low = 0, w_low = 0, replace = 1, final_paste = 0; float* loss = nullptr;
  // DDPM: K steps, tables of ones (never read before the first launch)
  float ones[K] = {1.f, 1.f, 1.f, 1.f}, zeros[K] = {0.f, 0.f, 0.f, 0.f};
  int32_t steps[K] = {0, 3, 5, 8}; int32_t walk[K + 3] = {4, 3, 2, 1, 0, 0, 0};
  mi355_ddpm_tables tb; mi355_ddpm_options opt; mi355_ddpm_schedule sd; mi355_multistep_schedule ms; mi355_x0_shaping sh;
  const mi355_ddpm_tables* tbp = &tb; const mi355_ddpm_options* optp = &opt; const mi355_ddpm_schedule* sdp = &sd;
  const mi355_multistep_schedule* msp = &ms; const mi355_x0_shaping* shp = &sh;
  const mi355_ddpm_schedule* shaped_sd = nullptr; const mi355_multistep_schedule* shaped_ms = nullptr;
  const float* noise = nullptr; int64_t n_draws = 0;

  Args(mi355_unet* n, mi355_unet* s, bool cc, int B) : net(n), score(s), classy(cc), batch(B) {
    tb = {K, ones, ones, ones, ones, zeros, ones, ones, ones, ones};
    opt = {}; opt.mode = cc ? MI355_DDPM_AMORTIZED : MI355_DDPM_PRIOR; opt.tmin = 1e-5f; opt.tmax = 1.f; opt.start_fraction = 1.f; opt.none_value = -2.f;
    sd = {steps, 10, nullptr, nullptr, 0, nullptr, nullptr};
    ms = {steps, 10, ones, ones, zeros};
    sh = {0.9f, 0.f, 0.f};
    if (cc) { cond = fake<float>(5); cond_channels = 3; labels = fake<int32_t>(8); }
  }
  Args(const Args&) = delete;   // it points into itself
};

// kind bits: what an entry point takes, and so which faults apply to it
enum { FLOW = 1, DDPM = 2, GUIDED = 4, TABLEAU = 8, AB = 16, SCHED = 32, MSCHED = 64, SHAPED = 128, UNCOND = 256, BATCH = 512 };
struct Entry {
  const char* name; int kind;
  void (*setup)(Args&);          // what the entry point needs beyond the plan's defaults (null: nothing)
  int (*call)(Args&);
  int64_t (*need)(const Args&);  // its workspace size function
};
void ddim(Args& a) { a.opt.mode = MI355_DDIM; }
#define SHAPED_CALL mi355_ddpm_shaped_sample(a.net, a.x, a.channels, a.cond, a.labels, a.null_label, a.guided, a.w, a.w_dev, a.tbp, a.optp, a.shaped_sd, \
                                             a.shaped_ms, a.shp, a.noise, a.n_draws, a.batch, a.ws, a.ws_bytes, nullptr)
const Entry entries[] = {
    {"cfm_euler_sample", FLOW, nullptr,
     [](Args& a) { return mi355_cfm_euler_sample(a.net, a.x, a.channels, a.cond, a.cond_channels, 0, a.ts, a.n_t, nullptr, nullptr, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_unet_workspace_bytes(a.net, a.batch); }},
    {"cfm_euler_sample_labels", FLOW, nullptr,
     [](Args& a) { return mi355_cfm_euler_sample_labels(a.net, a.x, a.channels, a.cond, a.cond_channels, 0, a.labels, a.ts, a.n_t, nullptr, nullptr, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_unet_workspace_bytes(a.net, a.batch); }},
    {"cfm_rk_sample", FLOW | TABLEAU | BATCH, nullptr,
     [](Args& a) { return mi355_cfm_rk_sample(a.net, a.x, a.channels, a.cond, a.cond_channels, a.labels, a.ts, a.n_t, a.stages, a.ap, a.bp, a.cp, nullptr, nullptr, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_cfm_rk_workspace_bytes(a.net, a.batch, a.stages); }},
    {"cfm_cfg_sample", FLOW | TABLEAU | GUIDED | BATCH, nullptr,
     [](Args& a) { return mi355_cfm_cfg_sample(a.net, a.x, a.channels, a.cond, a.cond_channels, a.none_value, a.labels, a.null_label, a.w, a.w_dev, a.ts, a.n_t, a.stages, a.ap, a.bp, a.cp, nullptr, nullptr, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_cfg_workspace_bytes(a.net, a.batch, a.stages); }},
    {"cfm_ab_sample", FLOW | TABLEAU | AB | BATCH, nullptr,
     [](Args& a) { return mi355_cfm_ab_sample(a.net, a.x, a.channels, a.cond, a.cond_channels, a.labels, a.ts, a.n_t, a.order, a.wp, a.stages, a.ap, a.bp, a.cp, nullptr, nullptr, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_cfm_ab_workspace_bytes(a.net, a.batch, a.order, a.stages, 0); }},
    {"cfm_ab_cfg_sample", FLOW | TABLEAU | AB | GUIDED | BATCH, nullptr,
     [](Args& a) { return mi355_cfm_ab_cfg_sample(a.net, a.x, a.channels, a.cond, a.cond_channels, a.none_value, a.labels, a.null_label, a.w, a.w_dev, a.ts, a.n_t, a.order, a.wp, a.stages, a.ap, a.bp, a.cp, nullptr, nullptr, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_cfm_ab_workspace_bytes(a.net, a.batch, a.order, a.stages, 1); }},
    {"cfm_recon_sample", FLOW | UNCOND | BATCH, nullptr,
     [](Args& a) { return mi355_cfm_recon_sample(a.net, a.x, a.channels, a.labels, a.ts, a.n_t, a.y, a.mode, -2.f, a.h_low, a.w_low, nullptr, a.replace, a.final_paste, nullptr, 0, nullptr, nullptr, a.loss, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_cfm_recon_workspace_bytes(a.net, a.batch, 0, 0); }},
    {"sf2m_euler_sample", FLOW | UNCOND | BATCH, nullptr,
     [](Args& a) { return mi355_sf2m_euler_sample(a.net, a.score, a.x, a.channels, a.labels, a.ts, a.n_t - 1, 0.3f, 0, nullptr, 7, nullptr, nullptr, 0, nullptr, a.batch, a.ws, a.ws_bytes, a.ws2, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_unet_workspace_bytes(a.net, a.batch); }},
    {"ddpm_sample", DDPM, nullptr,
     [](Args& a) { return mi355_ddpm_sample(a.net, a.x, a.channels, a.cond, a.tbp, a.optp, a.noise, a.n_draws, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_unet_workspace_bytes(a.net, a.batch); }},
    {"ddpm_sample_sched", DDPM | SCHED, nullptr,
     [](Args& a) { return mi355_ddpm_sample_sched(a.net, a.x, a.channels, a.cond, a.tbp, a.optp, a.sdp, a.noise, a.n_draws, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_unet_workspace_bytes(a.net, a.batch); }},
    {"ddpm_cfg_sample", DDPM | GUIDED | BATCH, nullptr,
     [](Args& a) { return mi355_ddpm_cfg_sample(a.net, a.x, a.channels, a.cond, a.labels, a.null_label, a.w, a.w_dev, a.tbp, a.optp, a.noise, a.n_draws, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_ddpm_cfg_workspace_bytes(a.net, a.batch); }},
    {"ddpm_cfg_sample_sched", DDPM | GUIDED | SCHED | BATCH, nullptr,
     [](Args& a) { return mi355_ddpm_cfg_sample_sched(a.net, a.x, a.channels, a.cond, a.labels, a.null_label, a.w, a.w_dev, a.tbp, a.optp, a.sdp, a.noise, a.n_draws, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_ddpm_cfg_workspace_bytes(a.net, a.batch); }},
    {"ddpm_multistep_sample", DDPM | MSCHED | BATCH, ddim,
     [](Args& a) { return mi355_ddpm_multistep_sample(a.net, a.x, a.channels, a.cond, a.tbp, a.optp, a.msp, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_ddpm_multistep_workspace_bytes(a.net, a.batch, 0); }},
    {"ddpm_multistep_cfg_sample", DDPM | GUIDED | MSCHED | BATCH, ddim,
     [](Args& a) { return mi355_ddpm_multistep_cfg_sample(a.net, a.x, a.channels, a.cond, a.labels, a.null_label, a.w, a.w_dev, a.tbp, a.optp, a.msp, a.batch, a.ws, a.ws_bytes, nullptr); },
     [](const Args& a) { return mi355_ddpm_multistep_workspace_bytes(a.net, a.batch, 1); }},
    {"ddpm_shaped_sample", DDPM | SHAPED | BATCH, nullptr, [](Args& a) { return SHAPED_CALL; },
     [](const Args& a) { return mi355_ddpm_shaped_workspace_bytes(a.net, a.batch, 0, 0); }},
    {"ddpm_shaped_sample sched", DDPM | SHAPED | SCHED | BATCH, [](Args& a) { a.shaped_sd = a.sdp; }, [](Args& a) { return SHAPED_CALL; },
     [](const Args& a) { return mi355_ddpm_shaped_workspace_bytes(a.net, a.batch, 0, 0); }},
    {"ddpm_shaped_sample guided", DDPM | SHAPED | GUIDED | BATCH, [](Args& a) { a.guided = 1; }, [](Args& a) { return SHAPED_CALL; },
     [](const Args& a) { return mi355_ddpm_shaped_workspace_bytes(a.net, a.batch, 1, 0); }},
    {"ddpm_shaped_sample msched", DDPM | SHAPED | MSCHED | BATCH, [](Args& a) { ddim(a); a.shaped_ms = a.msp; }, [](Args& a) { return SHAPED_CALL; },
     [](const Args& a) { return mi355_ddpm_shaped_workspace_bytes(a.net, a.batch, 0, 1); }},
    {"ddpm_shaped_sample guided msched", DDPM | SHAPED | GUIDED | MSCHED | BATCH, [](Args& a) { ddim(a); a.guided = 1; a.shaped_ms = a.msp; },
     [](Args& a) { return SHAPED_CALL; }, [](const Args& a) { return mi355_ddpm_shaped_workspace_bytes(a.net, a.batch, 1, 1); }},
};

// One fault each; make returns false where the fault does not apply to the entry point.  expect: what the refusal must say of the faulted argument
// (alternatives separated by |, one per wording among the entry points): a refusal in other words was made for another reason, so the fault was
// not the call's only one.  needs: kind bits an entry must have.
struct Fault { const char* name; const char* expect; int needs; bool (*make)(Args&, const Entry&); };
const Fault faults[] = {
    {"null net", "bad argument|null argument", 0, [](Args& a, const Entry&) { a.net = nullptr; return true; }},
    {"null x", "bad argument|null argument", 0, [](Args& a, const Entry&) { a.x = nullptr; return true; }},
    {"batch 0", "bad argument", BATCH, [](Args& a, const Entry&) { a.batch = 0; return true; }},
    {"wrong channels", "channel count", 0, [](Args& a, const Entry&) { a.channels = 4; return true; }},
    {"null workspace", "null argument|workspace, batch", 0, [](Args& a, const Entry&) { a.ws = nullptr; return true; }},
    {"misaligned workspace", "256-byte aligned", 0, [](Args& a, const Entry&) { a.ws = static_cast<char*>(a.ws) + 64; return true; }},
    {"workspace one byte short", "workspace too small", 0, [](Args& a, const Entry& e) { a.ws_bytes = e.need(a) - 1; return true; }},
    {"workspace of the unguided size", "workspace too small", GUIDED, [](Args& a, const Entry&) { a.ws_bytes = mi355_unet_workspace_bytes(a.net, a.batch); return true; }},
    {"labels without num_classes", "without num_classes", 0, [](Args& a, const Entry& e) { a.labels = fake<int32_t>(8); return !a.classy && !(e.kind & DDPM) && strcmp(e.name, "cfm_euler_sample") != 0; }},
    {"null_label out of range", "null_label", GUIDED, [](Args& a, const Entry&) { a.null_label = 10; return true; }},
    {"nothing to guide", "nothing to guide", GUIDED, [](Args& a, const Entry&) { a.labels = nullptr; a.cond = nullptr; return true; }},
    {"guided prior mode", "prior and replacement", GUIDED | DDPM, [](Args& a, const Entry& e) { a.opt.mode = MI355_DDPM_PRIOR; return !(e.kind & MSCHED); }},
    {"guided condition of 2 channels", "in_channels - out_channels", GUIDED | FLOW, [](Args& a, const Entry&) { a.cond_channels = 2; return true; }},
    {"null time span", "bad argument|t_span_host", FLOW, [](Args& a, const Entry&) { a.ts = nullptr; return true; }},
    {"n_t 0", "bad argument|t_span_host|n_t|n_steps", FLOW, [](Args& a, const Entry&) { a.n_t = 0; return true; }},
    {"5 stages", "1 to 4 stages", TABLEAU, [](Args& a, const Entry&) { a.stages = 5; return true; }},
    {"null tableau", "null tableau", TABLEAU, [](Args& a, const Entry&) { a.bp = nullptr; return true; }},
    {"all-zero b", "all zero", TABLEAU, [](Args& a, const Entry&) { a.b[1] = 0.f; return true; }},
    {"order 5", "order must be", AB, [](Args& a, const Entry&) { a.order = 5; return true; }},
    {"null w_host", "w_host is null", AB, [](Args& a, const Entry&) { a.wp = nullptr; return true; }},
    {"c_host[0] not 0", "c_host[0]", AB, [](Args& a, const Entry&) { a.c[0] = 0.5f; return true; }},
    {"all-zero weight row", "all-zero row", AB, [](Args& a, const Entry&) { a.wab[2] = a.wab[3] = 0.f; return true; }},
    {"recon mode 3", "mode must be", UNCOND, [](Args& a, const Entry& e) { a.mode = 3; return strcmp(e.name, "cfm_recon_sample") == 0; }},
    {"recon replace outside painting", "mode 0", UNCOND, [](Args& a, const Entry& e) { a.mode = 1; return strcmp(e.name, "cfm_recon_sample") == 0; }},
    {"recon final_paste without replace", "final_paste", UNCOND, [](Args& a, const Entry& e) { a.replace = 0; a.final_paste = 1; return strcmp(e.name, "cfm_recon_sample") == 0; }},
    {"recon replacement without y", "measurement y", UNCOND, [](Args& a, const Entry& e) { a.y = nullptr; return strcmp(e.name, "cfm_recon_sample") == 0; }},
    {"recon loss outside mode 2", "mode 2", UNCOND, [](Args& a, const Entry& e) { a.loss = fake<float>(9); return strcmp(e.name, "cfm_recon_sample") == 0; }},
    {"sf2m one workspace for both nets", "separate workspaces", UNCOND, [](Args& a, const Entry& e) { a.ws2 = a.ws; return strcmp(e.name, "sf2m_euler_sample") == 0; }},
    {"sf2m null score net", "bad argument", UNCOND, [](Args& a, const Entry& e) { a.score = nullptr; return strcmp(e.name, "sf2m_euler_sample") == 0; }},
    {"null tables", "null argument|bad argument|tables or opt", DDPM, [](Args& a, const Entry&) { a.tbp = nullptr; return true; }},
    {"null opt", "null argument|bad argument|tables or opt", DDPM, [](Args& a, const Entry&) { a.optp = nullptr; return true; }},
    {"replacement mode on this net", "replacement needs", DDPM, [](Args& a, const Entry& e) { a.opt.mode = MI355_DDPM_REPLACEMENT; return !(e.kind & (GUIDED | MSCHED)); }},
    {"amortized mode without a condition", "amortized needs", DDPM, [](Args& a, const Entry& e) { a.opt.mode = MI355_DDPM_AMORTIZED; a.cond = nullptr; return !(e.kind & (GUIDED | MSCHED)); }},
    {"null sched", "sched is null", SCHED, [](Args& a, const Entry& e) { a.sdp = nullptr; return !(e.kind & SHAPED); }},
    {"train_steps 0", "train_steps", SCHED, [](Args& a, const Entry&) { a.sd.train_steps = 0; return true; }},
    {"null steps", "steps is null", SCHED, [](Args& a, const Entry&) { a.sd.steps = nullptr; return true; }},
    {"steps not increasing", "strictly increasing", SCHED, [](Args& a, const Entry&) { a.steps[2] = 3; return true; }},
    {"ddim_sigma outside DDIM", "ddim_sigma belongs", SCHED, [](Args& a, const Entry&) { a.sd.ddim_sigma = a.zeros; return true; }},
    {"negative ddim_sigma", "ddim_sigma must be finite", SCHED, [](Args& a, const Entry&) { ddim(a); a.zeros[1] = -1.f; a.sd.ddim_sigma = a.zeros; return true; }},
    {"walk not from K", "start at level K", SCHED, [](Args& a, const Entry&) { a.sd.walk = a.walk + 1; a.sd.n_walk = K; return true; }},
    {"walk not to 0", "end at level 0", SCHED, [](Args& a, const Entry&) { a.sd.walk = a.walk; a.sd.n_walk = K; return true; }},
    {"walk jumps", "+-1", SCHED, [](Args& a, const Entry&) { a.walk[1] = 2; a.walk[2] = 1; a.walk[3] = 0; a.sd.walk = a.walk; a.sd.n_walk = 4; return true; }},
    {"walk up without renoise (guided: walk up)", "upward moves", SCHED, [](Args& a, const Entry&) {
       const int32_t up[7] = {4, 3, 4, 3, 2, 1, 0}; memcpy(a.walk, up, sizeof up); a.sd.walk = a.walk; a.sd.n_walk = 7; return true; }},
    {"null msched", "msched is null", MSCHED, [](Args& a, const Entry& e) { a.msp = nullptr; return !(e.kind & SHAPED); }},
    {"multistep outside DDIM", "must be MI355_DDIM", MSCHED, [](Args& a, const Entry&) { a.opt.mode = a.classy ? MI355_DDPM_AMORTIZED : MI355_DDPM_PRIOR; return true; }},
    {"multistep train_steps 0", "train_steps", MSCHED, [](Args& a, const Entry&) { a.ms.train_steps = 0; return true; }},
    {"null cx", "cx is null", MSCHED, [](Args& a, const Entry&) { a.ms.cx = nullptr; return true; }},
    {"null c0", "c0 is null", MSCHED, [](Args& a, const Entry&) { a.ms.c0 = nullptr; return true; }},
    {"null c1", "c1 is null", MSCHED, [](Args& a, const Entry&) { a.ms.c1 = nullptr; return true; }},
    {"c0 not finite", "c0 must be finite", MSCHED, [](Args& a, const Entry&) { a.t_span[1] = __builtin_inff(); a.ms.c0 = a.t_span; return true; }},
    {"c1[K-1] not 0", "c1[K-1]", MSCHED, [](Args& a, const Entry&) { a.ms.c1 = a.ones; return true; }},
    {"quantile 2", "quantile", SHAPED, [](Args& a, const Entry&) { a.sh.quantile = 2.f; return true; }},
    {"max_threshold 0.5", "max_threshold", SHAPED, [](Args& a, const Entry&) { a.sh.max_threshold = 0.5f; return true; }},
    {"rescale_phi 2", "rescale_phi must be in", SHAPED, [](Args& a, const Entry&) { a.sh.rescale_phi = 2.f; return true; }},
    {"rescale_phi unguided", "needs guided", SHAPED, [](Args& a, const Entry& e) { a.sh.rescale_phi = 0.5f; return !(e.kind & GUIDED); }},
    {"sched and msched", "both sched and msched", SHAPED, [](Args& a, const Entry&) { a.shaped_sd = a.sdp; a.shaped_ms = a.msp; return true; }},
    {"noise with msched", "noise given with msched", SHAPED | MSCHED, [](Args& a, const Entry&) { a.noise = fake<float>(9); a.n_draws = 8; return true; }},
};

// The predictor-step exports (one launcher behind all ten): what each form refuses before its launch.
struct StepCase { const char* name; const char* expect; int (*call)(); };
float* const X = fake<float>(3); float* const E = fake<float>(4); float* const H = fake<float>(5); float* const WD = fake<float>(6); float* const SHP = fake<float>(7);
const StepCase step_cases[] = {
    {"ddpm_step | offset 2", "Philox offset", [] { return mi355_ddpm_step(X, E, nullptr, 1.f, 1.f, 1.f, 1.f, 1.f, 1, 7, 2, 64, nullptr); }},
    {"ddpm_cfg_step | offset 2", "Philox offset", [] { return mi355_ddpm_cfg_step(X, E, nullptr, 2.f, nullptr, 32, 1.f, 1.f, 1.f, 1.f, 1.f, 1, 7, 2, 64, nullptr); }},
    {"ddpm_cfg_step | w_dev with elems_per_image 0", "per-image scales", [] { return mi355_ddpm_cfg_step(X, E, nullptr, 2.f, WD, 0, 1.f, 1.f, 1.f, 1.f, 1.f, 1, 7, 0, 64, nullptr); }},
    {"ddpm_cfg_step | null eps", "null argument", [] { return mi355_ddpm_cfg_step(X, nullptr, nullptr, 2.f, nullptr, 32, 1.f, 1.f, 1.f, 1.f, 1.f, 1, 7, 0, 64, nullptr); }},
    {"ddim_cfg_step | w_dev over part images", "per-image scales", [] { return mi355_ddim_cfg_step(X, E, 2.f, WD, 48, 1.f, 1.f, 0.5f, 64, nullptr); }},
    {"ddim_cfg_step | null x", "null argument", [] { return mi355_ddim_cfg_step(nullptr, E, 2.f, nullptr, 32, 1.f, 1.f, 0.5f, 64, nullptr); }},
    {"ddim_eta_step | offset 2", "Philox offset", [] { return mi355_ddim_eta_step(X, E, nullptr, 1.f, 1.f, 0.5f, 0.1f, 1, 7, 2, 64, nullptr); }},
    {"ddim_eta_step | null eps", "null argument", [] { return mi355_ddim_eta_step(X, nullptr, nullptr, 1.f, 1.f, 0.5f, 0.1f, 1, 7, 0, 64, nullptr); }},
    {"ddim_eta_step | sigma -1", "sigma must be", [] { return mi355_ddim_eta_step(X, E, nullptr, 1.f, 1.f, 0.5f, -1.f, 1, 7, 0, 64, nullptr); }},
    {"ddim_eta_cfg_step | offset 2", "Philox offset", [] { return mi355_ddim_eta_cfg_step(X, E, nullptr, 2.f, nullptr, 32, 1.f, 1.f, 0.5f, 0.1f, 1, 7, 2, 64, nullptr); }},
    {"ddim_eta_cfg_step | w_dev with elems_per_image 0", "per-image scales", [] { return mi355_ddim_eta_cfg_step(X, E, nullptr, 2.f, WD, 0, 1.f, 1.f, 0.5f, 0.1f, 1, 7, 0, 64, nullptr); }},
    {"ddim_eta_cfg_step | null x", "null argument", [] { return mi355_ddim_eta_cfg_step(nullptr, E, nullptr, 2.f, nullptr, 32, 1.f, 1.f, 0.5f, 0.1f, 1, 7, 0, 64, nullptr); }},
    {"ddim_eta_cfg_step | sigma not finite", "sigma must be", [] { return mi355_ddim_eta_cfg_step(X, E, nullptr, 2.f, nullptr, 32, 1.f, 1.f, 0.5f, __builtin_inff(), 1, 7, 0, 64, nullptr); }},
    {"dpmpp_step | null eps", "null argument", [] { return mi355_dpmpp_step(X, nullptr, H, 1.f, 1.f, 1.f, 1.f, 0.f, 64, nullptr); }},
    {"dpmpp_step | c1 without hist", "needs hist", [] { return mi355_dpmpp_step(X, E, nullptr, 1.f, 1.f, 1.f, 1.f, 0.5f, 64, nullptr); }},
    {"dpmpp_cfg_step | w_dev with elems_per_image 0", "per-image scales", [] { return mi355_dpmpp_cfg_step(X, E, H, 2.f, WD, 0, 1.f, 1.f, 1.f, 1.f, 0.f, 64, nullptr); }},
    {"dpmpp_cfg_step | null x", "null argument", [] { return mi355_dpmpp_cfg_step(nullptr, E, H, 2.f, nullptr, 32, 1.f, 1.f, 1.f, 1.f, 0.f, 64, nullptr); }},
    {"dpmpp_cfg_step | c1 without hist", "needs hist", [] { return mi355_dpmpp_cfg_step(X, E, nullptr, 2.f, nullptr, 32, 1.f, 1.f, 1.f, 1.f, 0.5f, 64, nullptr); }},
    {"x0_shaped_step | kind 4", "kind must be", [] { return mi355_x0_shaped_step(4, X, E, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, 1.f, 1.f, 0.f, 0.f, 1, 7, 0, SHP, 64, nullptr); }},
    {"x0_shaped_step | elems_per_image 0", "whole images", [] { return mi355_x0_shaped_step(1, X, E, nullptr, H, 0, 0.f, nullptr, 0, 1.f, 1.f, 1.f, 1.f, 0.f, 0.f, 1, 7, 0, SHP, 64, nullptr); }},
    {"x0_shaped_step | part images", "whole images", [] { return mi355_x0_shaped_step(1, X, E, nullptr, H, 0, 0.f, nullptr, 48, 1.f, 1.f, 1.f, 1.f, 0.f, 0.f, 1, 7, 0, SHP, 64, nullptr); }},
    {"x0_shaped_step | ancestral, offset 2", "Philox offset", [] { return mi355_x0_shaped_step(0, X, E, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, 1.f, 1.f, 0.f, 1.f, 1, 7, 2, SHP, 64, nullptr); }},
    {"x0_shaped_step | guided DDIM(eta), sigma -1", "sigma must be", [] { return mi355_x0_shaped_step(2, X, E, nullptr, H, 1, 2.f, nullptr, 32, 1.f, 1.f, 0.5f, 0.f, 0.f, -1.f, 1, 7, 0, SHP, 64, nullptr); }},
    {"x0_shaped_step | guided DPM-Solver++, c1 without hist", "needs hist", [] { return mi355_x0_shaped_step(3, X, E, nullptr, nullptr, 1, 2.f, nullptr, 32, 1.f, 1.f, 1.f, 1.f, 0.5f, 0.f, 0, 0, 0, SHP, 64, nullptr); }},
    {"x0_shaped_step | guided DDIM, null eps", "null argument", [] { return mi355_x0_shaped_step(1, X, nullptr, nullptr, H, 1, 2.f, nullptr, 32, 1.f, 1.f, 0.5f, 0.f, 0.f, 0.f, 0, 0, 0, SHP, 64, nullptr); }},
    {"x0_shape_stats | quantile 2", "quantile", [] { const mi355_x0_shaping sh{2.f, 0.f, 0.f}; return mi355_x0_shape_stats(X, E, 0.f, nullptr, 0, 1.f, 1.f, &sh, SHP, nullptr, 2, 32, nullptr); }},
    {"x0_shape_stats | null shape", "shape is null", [] { const mi355_x0_shaping sh{0.9f, 0.f, 0.f}; return mi355_x0_shape_stats(X, E, 0.f, nullptr, 0, 1.f, 1.f, &sh, nullptr, nullptr, 2, 32, nullptr); }},
    {"x0_shape_stats | batch 0", "batch must be", [] { const mi355_x0_shaping sh{0.9f, 0.f, 0.f}; return mi355_x0_shape_stats(X, E, 0.f, nullptr, 0, 1.f, 1.f, &sh, SHP, nullptr, 0, 32, nullptr); }},
    // x0- and v-prediction nets: the ops that take the kind, and the two entry points' refusals that need no handle
    {"pred_step | kind 6", "kind must be", [] { return mi355_pred_step(6, 1, X, E, 0, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 1, 7, 0, nullptr, 64, nullptr); }},
    {"pred_step | pred_kind 3", "pred_kind must be", [] { return mi355_pred_step(1, 3, X, E, 0, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 1, 7, 0, nullptr, 64, nullptr); }},
    {"pred_step | pred_kind -1, corrector", "pred_kind must be", [] { return mi355_pred_step(4, -1, X, E, 0, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 1, 7, 0, nullptr, 64, nullptr); }},
    {"pred_step | part images", "whole images", [] { return mi355_pred_step(0, 2, X, E, 0, nullptr, H, 0, 0.f, nullptr, 48, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 1, 7, 0, nullptr, 64, nullptr); }},
    {"pred_step | out_stride under elems_per_image", "out_stride", [] { return mi355_pred_step(1, 2, X, E, 8, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 1, 7, 0, nullptr, 64, nullptr); }},
    {"pred_step | guided corrector", "no guided form", [] { return mi355_pred_step(4, 2, X, E, 0, nullptr, H, 1, 2.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 1, 7, 0, nullptr, 64, nullptr); }},
    {"pred_step | shaped corrector", "static clip", [] { return mi355_pred_step(4, 1, X, E, 0, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 1, 7, 0, SHP, 64, nullptr); }},
    {"pred_step | v, ancestral, offset 2", "Philox offset", [] { return mi355_pred_step(0, 2, X, E, 0, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 1.f, -3.f, -1.f, 1, 7, 2, nullptr, 64, nullptr); }},
    {"pred_step | x0, learned variance on a narrow output", "variance channels sit behind", [] { return mi355_pred_step(5, 1, X, E, 32, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 1, 7, 0, nullptr, 64, nullptr); }},
    {"pred_step | v, shaped on a strided output", "strided eps", [] { return mi355_pred_step(1, 2, X, E, 64, nullptr, H, 0, 0.f, nullptr, 32, 1.f, 1.f, .8f, .6f, .5f, 0.f, 0.f, 0.f, -3.f, -1.f, 0, 0, 0, SHP, 64, nullptr); }},
    {"pred_step | x0, guided DPM-Solver++, null out", "null argument", [] { return mi355_pred_step(3, 1, X, nullptr, 0, nullptr, H, 1, 2.f, nullptr, 32, 1.f, 1.f, .8f, .6f, 1.f, 1.f, 0.f, 0.f, -3.f, -1.f, 0, 0, 0, nullptr, 64, nullptr); }},
    {"pred_shape_stats | pred_kind 3", "prediction kind must be", [] { const mi355_x0_shaping sh{0.9f, 0.f, 0.f}; return mi355_pred_shape_stats(3, X, E, 0.f, nullptr, 0, 1.f, 1.f, .8f, .6f, &sh, SHP, nullptr, 2, 32, nullptr); }},
    {"pred_shape_stats | v, null x", "x is null", [] { const mi355_x0_shaping sh{0.9f, 0.f, 0.f}; return mi355_pred_shape_stats(2, nullptr, E, 0.f, nullptr, 0, 1.f, 1.f, .8f, .6f, &sh, SHP, nullptr, 2, 32, nullptr); }},
    {"pred_shape_stats | x0, null x, null shape", "shape is null", [] { const mi355_x0_shaping sh{0.9f, 0.f, 0.f}; return mi355_pred_shape_stats(1, nullptr, E, 0.f, nullptr, 0, 1.f, 1.f, .8f, .6f, &sh, nullptr, nullptr, 2, 32, nullptr); }},
    {"vlb_terms_pred | pred_kind 3", "prediction kind must be", [] { return mi355_vlb_terms_pred(X, X, E, 32, nullptr, 1, 7, 0, 1.f, 1.f, .5f, .5f, -3.f, -3.f, -3.f, -1.f, 0, 0, 0, 1, 3, .8f, .6f, SHP, 3, 2, 32, nullptr); }},
    {"vlb_terms_pred | v, sb not finite", "sa and sb must be finite", [] { return mi355_vlb_terms_pred(X, X, E, 32, nullptr, 1, 7, 0, 1.f, 1.f, .5f, .5f, -3.f, -3.f, -3.f, -1.f, 0, 0, 0, 1, 2, .8f, __builtin_nanf(""), SHP, 3, 2, 32, nullptr); }},
    {"vlb_terms_pred | x0, no draw", "the step's draw is needed", [] { return mi355_vlb_terms_pred(X, X, E, 32, nullptr, 0, 7, 0, 1.f, 1.f, .5f, .5f, -3.f, -3.f, -3.f, -1.f, 0, 0, 0, 1, 1, .8f, .6f, SHP, 3, 2, 32, nullptr); }},
    {"ddpm_pred_sample | pred->kind 3", "pred->kind must be", [] { float t[K] = {1.f, 1.f, 1.f, 1.f}; const mi355_ddpm_tables tb{K, t, t, t, t, t, t, t, t, t}; const mi355_ddpm_options o{};
       const mi355_ddpm_prediction p{3}; return mi355_ddpm_pred_sample(nullptr, X, 3, nullptr, nullptr, 0, 0, 0.f, nullptr, &tb, &o, nullptr, nullptr, nullptr, nullptr, &p, nullptr, 0, 2, H, 1 << 20, nullptr); }},
    {"ddpm_pred_sample | v without its tables", "needs tables->sqrt_alphas_cumprod", [] { float t[K] = {1.f, 1.f, 1.f, 1.f}; const mi355_ddpm_tables tb{K, t, t, t, t, t, nullptr, t, t, t};
       const mi355_ddpm_options o{}; const mi355_ddpm_prediction p{2};
       return mi355_ddpm_pred_sample(nullptr, X, 3, nullptr, nullptr, 0, 0, 0.f, nullptr, &tb, &o, nullptr, nullptr, nullptr, nullptr, &p, nullptr, 0, 2, H, 1 << 20, nullptr); }},
    {"ddpm_pred_sample | x0, learned variance with shaping", "var->learned together with shaping", [] { float t[K] = {1.f, 1.f, 1.f, 1.f}; const mi355_ddpm_tables tb{K, t, t, t, t, t, t, t, t, t};
       const mi355_ddpm_options o{}; const mi355_ddpm_prediction p{1}; const mi355_ddpm_variance v{1, t, nullptr}; const mi355_x0_shaping sh{0.9f, 0.f, 0.f};
       return mi355_ddpm_pred_sample(nullptr, X, 3, nullptr, nullptr, 0, 0, 0.f, nullptr, &tb, &o, nullptr, nullptr, &v, &sh, &p, nullptr, 0, 2, H, 1 << 20, nullptr); }},
    {"ddpm_pred_sample | v, no handle", "bad argument (net, x, workspace, batch)", [] { float t[K] = {1.f, 1.f, 1.f, 1.f}; const mi355_ddpm_tables tb{K, t, t, t, t, t, t, t, t, t};
       const mi355_ddpm_options o{}; const mi355_ddpm_prediction p{2};
       return mi355_ddpm_pred_sample(nullptr, X, 3, nullptr, nullptr, 0, 0, 0.f, nullptr, &tb, &o, nullptr, nullptr, nullptr, nullptr, &p, nullptr, 0, 2, H, 1 << 20, nullptr); }},
    {"ddpm_vlb_pred | pred->kind -1", "pred->kind must be", [] { float t[K] = {1.f, 1.f, 1.f, 1.f}; const mi355_ddpm_tables tb{K, t, t, t, t, t, t, t, t, t}; const mi355_ddpm_prediction p{-1};
       return mi355_ddpm_vlb_pred(nullptr, X, 3, nullptr, nullptr, &tb, nullptr, &p, nullptr, 0, E, H, 2, SHP, 1 << 20, nullptr); }},
    {"ddpm_vlb_pred | v, opt null", "opt is null", [] { float t[K] = {1.f, 1.f, 1.f, 1.f}; const mi355_ddpm_tables tb{K, t, t, t, t, t, t, t, t, t}; const mi355_ddpm_prediction p{2};
       return mi355_ddpm_vlb_pred(nullptr, X, 3, nullptr, nullptr, &tb, nullptr, &p, nullptr, 0, E, H, 2, SHP, 1 << 20, nullptr); }},
};

// the text of the refusal just made says one of the |-separated alternatives
bool says(const char* alternatives) {
  const std::string text = mi355_last_error(), alts = alternatives;
  for (size_t i = 0; i <= alts.size();) {
    const size_t j = alts.find('|', i) == std::string::npos ? alts.size() : alts.find('|', i);
    if (text.find(alts.substr(i, j - i)) != std::string::npos) return true;
    i = j + 1;
  }
  return false;
}
// one line of the record; a case fails if the call was accepted (0), got as far as a HIP call (-3), or was refused in other words than expected
int report(const char* entry, const char* what, const char* expect, int rc) {
  printf("  %s | %s | %d | %s\n", entry, what, rc, rc ? mi355_last_error() : "");
  if (rc != 0 && rc != -3 && says(expect)) return 0;
  printf("  ^ FAILED: %s\n", rc == 0 || rc == -3 ? "not refused on the host" : "refused for another reason than the fault made");
  return 1;
}

// The variational bound: its workspace is the plain sampler's, and every refusal of mi355_ddpm_vlb comes before the first launch, one fault each.
int vlb_cases(mi355_unet* net, bool cc, int B) {
  const int64_t need = mi355_ddpm_vlb_workspace_bytes(net, B);
  printf("  bytes ddpm_vlb_workspace %lld\n", (long long)need);
  int bad = need != mi355_unet_workspace_bytes(net, B);
  if (bad) printf("  ^ FAILED: the bound's workspace is not the plain sampler's\n");
  struct Case {
    const char* what; const char* expect;
    int learned = 0, cdf = 0, clip = 1, Ns = K, channels = 3; int64_t ws_bytes = int64_t(1) << 50, n_draws = 0;
    bool no_true = false, no_model = false, no_min = false, bad_true = false, bad_chain = false, bad_times = false, cond = false, labels = false, noise = false,
         no_x0 = false, no_terms = false, no_summary = false, no_ws = false, no_tb = false, no_opt = false, no_net = false;
  };
  const auto mk = [](const char* what, const char* expect) { Case c; c.what = what; c.expect = expect; return c; };
  Case cases[24];
  int n = 0;
  { Case c = mk("tables null", "tables is null"); c.no_tb = true; cases[n++] = c; }
  { Case c = mk("opt null", "opt is null"); c.no_opt = true; cases[n++] = c; }
  { Case c = mk("one step", "Ns must be >= 2"); c.Ns = 1; cases[n++] = c; }
  { Case c = mk("learned 2", "opt->learned"); c.learned = 2; cases[n++] = c; }
  { Case c = mk("cdf 2", "opt->cdf"); c.cdf = 2; cases[n++] = c; }
  { Case c = mk("clip_denoised -1", "opt->clip_denoised"); c.clip = -1; cases[n++] = c; }
  { Case c = mk("true_log null", "opt->true_log is null"); c.no_true = true; cases[n++] = c; }
  { Case c = mk("model_log null, fixed", "opt->model_log is null"); c.no_model = true; cases[n++] = c; }
  { Case c = mk("min_log null, learned", "opt->min_log is null"); c.learned = 1; c.no_min = true; cases[n++] = c; }
  { Case c = mk("true_log not finite", "opt->true_log must be finite"); c.bad_true = true; cases[n++] = c; }
  { Case c = mk("a chain table not finite", "tables->posterior_mean_coef1 must be finite"); c.bad_chain = true; cases[n++] = c; }
  { Case c = mk("times not finite", "opt->times must be finite"); c.bad_times = true; cases[n++] = c; }
  { Case c = mk("net null", "net is null"); c.no_net = true; cases[n++] = c; }
  { Case c = mk("x0 null", "x0 is null"); c.no_x0 = true; cases[n++] = c; }
  { Case c = mk("out_terms null", "out_terms is null"); c.no_terms = true; cases[n++] = c; }
  { Case c = mk("summary null", "summary is null"); c.no_summary = true; cases[n++] = c; }
  { Case c = mk("workspace null", "workspace is null"); c.no_ws = true; cases[n++] = c; }
  { Case c = mk("learned on a C-output net", "out_channels == 2 * channels"); c.learned = 1; cases[n++] = c; }
  { Case c = mk("fixed with the wrong channel count", "out_channels == channels"); c.channels = 1; cases[n++] = c; }
  if (!cc) { Case c = mk("cond on a net that takes none", "takes no condition"); c.cond = true; cases[n++] = c; }
  if (!cc) { Case c = mk("labels on a net without classes", "without num_classes"); c.labels = true; cases[n++] = c; }
  { Case c = mk("too few injected draws", "injected noise exhausted"); c.noise = true; c.n_draws = K - 1; cases[n++] = c; }
  { Case c = mk("workspace one byte short", "workspace too small"); c.ws_bytes = need - 1; cases[n++] = c; }
  for (int i = 0; i < n; ++i) {
    const Case& c = cases[i];
    float fine[K] = {-3.f, -2.5f, -2.f, -1.f}, nanful[K] = {-3.f, NAN, -2.f, -1.f}, ones[K] = {1.f, 1.f, 1.f, 1.f}, half[K] = {0.5f, 0.5f, 0.5f, 0.5f},
          inff[K] = {1.f, 1.f, INFINITY, 1.f};
    const mi355_ddpm_tables tb{c.Ns, ones, ones, c.bad_chain ? inff : ones, ones, fine, half, half, ones, ones};
    mi355_vlb_options o{};
    o.learned = c.learned; o.cdf = c.cdf; o.clip_denoised = c.clip;
    o.true_log = c.no_true ? nullptr : (c.bad_true ? nanful : fine);
    o.model_log = c.no_model ? nullptr : fine; o.min_log = c.no_min ? nullptr : fine; o.max_log = fine;
    o.times = c.bad_times ? nanful : nullptr; o.none_value = -2.f; o.seed = 1;
    const int rc = mi355_ddpm_vlb(c.no_net ? nullptr : net, c.no_x0 ? nullptr : fake<float>(3), c.channels, (c.cond || cc) ? fake<float>(5) : nullptr,
                                  (c.labels || cc) ? fake<int32_t>(8) : nullptr, c.no_tb ? nullptr : &tb, c.no_opt ? nullptr : &o,
                                  c.noise ? fake<float>(9) : nullptr, c.n_draws, c.no_terms ? nullptr : fake<float>(10), c.no_summary ? nullptr : fake<float>(11),
                                  B, c.no_ws ? nullptr : fake<void>(2), c.ws_bytes, nullptr);
    bad += report("mi355_ddpm_vlb", c.what, c.expect, rc);
  }
  return bad;
}

// Tiled sampling: the workspace rule (the sampler workspace at batch `chunk`, then the window buffers the net reads and writes, the blended
// canvas and the repeated labels) and the refusals of the three entry points, one fault each.
int tiled_cases(mi355_unet* net, bool cc, int B) {
  const mi355_unet_config& c = net->cfg;
  const int S = c.image_size;
  const mi355_tile_plan good{2 * S, 3 * S - 5, S / 2, S / 3, MI355_TILE_TENT, 4};
  int32_t cnt[3] = {0, 0, 0};
  int bad = mi355_tile_count(S, &good, cnt) != 0;
  const int64_t need = mi355_tiled_workspace_bytes(net, B, &good), plain = mi355_unet_workspace_bytes(net, good.chunk);
  const int64_t rows = (int64_t)B * cnt[2], hw = (int64_t)S * S;
  const int64_t parts = rows * (c.in_channels + c.out_channels) * hw * 4 + (int64_t)B * c.out_channels * good.canvas_h * good.canvas_w * 4;
  printf("  bytes tiled_workspace %lld (windows %d x %d; plain at chunk %lld + window and canvas buffers %lld)\n", (long long)need, cnt[0], cnt[1],
         (long long)plain, (long long)parts);
  if (need < plain + parts) { printf("  ^ FAILED: the tiled workspace is smaller than its parts\n"); ++bad; }
  struct Case { const char* what; const char* expect; mi355_tile_plan plan; int64_t ws_bytes; int cond_drift; };
  const int64_t big = int64_t(1) << 50;
  const Case cases[] = {
      {"canvas_h below image_size", "canvas_h", {S - 1, 2 * S, 8, 8, 0, 4}, big, 0},
      {"canvas_w below image_size", "canvas_w", {2 * S, S - 1, 8, 8, 0, 4}, big, 0},
      {"stride_y 0", "stride_y", {2 * S, 2 * S, 0, 8, 0, 4}, big, 0},
      {"stride_x above image_size", "stride_x", {2 * S, 2 * S, 8, S + 1, 0, 4}, big, 0},
      {"unknown weight", "weight", {2 * S, 2 * S, 8, 8, 7, 4}, big, 0},
      {"chunk 0", "chunk", {2 * S, 2 * S, 8, 8, 0, 0}, big, 0},
      {"chunk above the largest batch", "chunk is above", {2 * S, 2 * S, 8, 8, 0, 1 << 30}, big, 0},
      {"workspace one byte short", "workspace too small", good, need - 1, 0},
  };
  Args a(net, net, cc, B);
  for (const Case& k : cases) {
    bad += report("unet_forward_tiled", k.what, k.expect,
                  mi355_unet_forward_tiled(net, a.x, 3, a.cond, a.cond_channels, 0.5f, a.labels, fake<float>(9), B, &k.plan, a.ws, k.ws_bytes, nullptr));
    bad += report("cfm_euler_sample_tiled", k.what, k.expect,
                  mi355_cfm_euler_sample_tiled(net, a.x, 3, a.cond, a.cond_channels, 0, a.labels, a.ts, a.n_t, nullptr, nullptr, B, a.ws, k.ws_bytes, nullptr,
                                               &k.plan));
    bad += report("ddpm_sample_tiled", k.what, k.expect,
                  mi355_ddpm_sample_tiled(net, a.x, 3, a.cond, a.tbp, a.optp, nullptr, nullptr, 0, B, a.ws, k.ws_bytes, nullptr, &k.plan));
    if (k.ws_bytes == big) bad += report("tiled_workspace_bytes", k.what, k.expect, (int)mi355_tiled_workspace_bytes(net, B, &k.plan));
  }
  bad += report("cfm_euler_sample_tiled", "cond_drift", "cond_drift",
                mi355_cfm_euler_sample_tiled(net, a.x, 3, a.cond, a.cond_channels, 1, a.labels, a.ts, a.n_t, nullptr, nullptr, B, a.ws, big, nullptr, &good));
  bad += report("cfm_euler_sample_tiled", "null plan", "plan is null",
                mi355_cfm_euler_sample_tiled(net, a.x, 3, a.cond, a.cond_channels, 0, a.labels, a.ts, a.n_t, nullptr, nullptr, B, a.ws, big, nullptr, nullptr));
  return bad;
}

int run_plan(const char* name, const mi355_unet_config& cfg, int B) {
  mi355_unet net, score;
  if (unet_plan_dry(cfg, &net) < 0 || unet_plan_dry(cfg, &score) < 0) { fprintf(stderr, "%s: plan failed: %s\n", name, mi355_last_error()); return 1; }
  net.dev_weights = score.dev_weights = fake<char>(1);
  const bool cc = cfg.num_classes > 0;
  printf("%s B=%d\n", name, B);
  printf("  bytes unet_workspace %lld\n", (long long)mi355_unet_workspace_bytes(&net, B));
  printf("  bytes ddpm_cfg_workspace %lld\n", (long long)mi355_ddpm_cfg_workspace_bytes(&net, B));
  for (int st = 1; st <= 4; ++st)
    printf("  bytes stages=%d cfm_rk_workspace %lld cfg_workspace %lld\n", st, (long long)mi355_cfm_rk_workspace_bytes(&net, B, st),
           (long long)mi355_cfg_workspace_bytes(&net, B, st));
  for (int g = 0; g <= 1; ++g) {
    printf("  bytes guided=%d ddpm_multistep_workspace %lld ddpm_shaped_workspace %lld ddpm_shaped_workspace(multistep) %lld\n", g,
           (long long)mi355_ddpm_multistep_workspace_bytes(&net, B, g), (long long)mi355_ddpm_shaped_workspace_bytes(&net, B, g, 0),
           (long long)mi355_ddpm_shaped_workspace_bytes(&net, B, g, 1));
    for (int order = 2; order <= 4; ++order)
      for (int st = 1; st <= 4; ++st)
        printf("  bytes guided=%d order=%d start_stages=%d cfm_ab_workspace %lld\n", g, order, st, (long long)mi355_cfm_ab_workspace_bytes(&net, B, order, st, g));
  }
  for (int hl : {0, 8}) printf("  bytes h_low=w_low=%d cfm_recon_workspace %lld\n", hl, (long long)mi355_cfm_recon_workspace_bytes(&net, B, hl, hl));
  int bad = 0;
  for (const Entry& e : entries) {
    // A guided entry point refuses the plain plan whatever else is asked (nothing to guide), the unconditional samplers the amortized one: that
    // refusal is the entry point's one case there.  No call is made that the host checks accept: it would go on to HIP calls on made-up addresses.
    if (((e.kind & GUIDED) && !cc) || ((e.kind & UNCOND) && cc)) {
      Args a(&net, &score, cc, B);
      if (e.setup) e.setup(a);
      bad += report(e.name, "the plan itself", cc ? "unconditional net|map the state's channel count" : "nothing to guide|prior and replacement", e.call(a));
      continue;
    }
    for (const Fault& f : faults) {
      if ((e.kind & f.needs) != f.needs) continue;
      Args a(&net, &score, cc, B);
      if (e.setup) e.setup(a);
      if (!f.make(a, e)) continue;
      bad += report(e.name, f.name, f.expect, e.call(a));
    }
  }
  bad += tiled_cases(&net, cc, B);
  bad += vlb_cases(&net, cc, B);
  return bad;
}

}  // namespace

int main() {
  // Every call below is meant to be refused on the host; one that is not would reach HIP with made-up addresses.  Where a GPU driver is present
  // that is a memory fault on a device others may share, so the program does not run there at all.
  if (access("/dev/kfd", F_OK) == 0) {
    fprintf(stderr, "sampler_refusals: this machine has a GPU driver node (/dev/kfd); the program runs on machines without a device only\n");
    return 2;
  }
  int bad = 0;
  printf("predictor steps\n");
  for (const StepCase& c : step_cases) bad += report("step", c.name, c.expect, c.call());
  for (int B : {3, 8}) {
    bad += run_plan("cifar", cifar(), B);
    bad += run_plan("classcond", classcond(), B);
  }
  if (bad) fprintf(stderr, "%d cases failed\n", bad);
  return bad ? 1 : 0;
}
