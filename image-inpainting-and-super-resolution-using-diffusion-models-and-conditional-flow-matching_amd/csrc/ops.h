// Internal C++ launch API shared by the U-Net executor, the sampler loops and the C ABI.
#pragma once
#include "common.h"
#include "../../include/mi355_sampler.h"

const mi355_debug_config& mi355_default_debug();   // the shipped behaviour (capi.hip)

// INTERNAL element-type codes of every descriptor below (the C ABI's MI355_* dtype values are translated at the boundary, capi.hip and test_ops.hip: MI355_BF16X2 ->
// DT_BF16 + ConvDesc::wsplit, MI355_F16 -> DT_F16).  Sizes and chunking depend only on "4-byte or 2-byte": dtype == 0 ? 4 : 2.
enum { DT_F32 = 0, DT_BF16 = 1, DT_F16 = 2 };
// run f(T()) for the element type of an internal dtype code
template <typename F> auto dispatch_dtype(int dtype, F&& f) {
  if (dtype == DT_F32) return f(float());
  if (dtype == DT_F16) return f(f16());
  return f(bf16());
}

// ---- implicit-GEMM convolution -------------------------------------------------------------------
// Activations are NHWC in HBM ([N][H][W][C], element type float or bf16).  out[n, y, x, co] =
//   bias[co] + emb[n, co] + res[...] + sum_{tap, ci} W[co, ci, tap] * P(in)[n, y*s + ky - pad, x*s + kx - pad, ci]
// where P is the optional fused prologue  P(v) = silu?(a[n, ci] * v + b[n, ci])  (GroupNorm affine,
// FiLM folded into a/b) evaluated while the input patch is staged into LDS, and `in` is read through
// a gather: identity | nearest x2 upsample | 2x2 average pool (both applied AFTER P, as the reference
// does: ResBlock up/down resamples between SiLU and the conv, unet.py:332-337).
enum ConvMode { CONV_UNIT = 0, CONV_STRIDE2 = 1, CONV_UP2 = 2, CONV_POOL2 = 3 };
enum ResMode { RES_NONE = 0, RES_SAME = 1, RES_UP2 = 2, RES_POOL2 = 3 };
enum OutMode { OUT_NHWC = 0, OUT_NCHW_F32 = 1 };

struct ConvDesc {
  int dtype;                 // MI355_F32 / MI355_BF16
  const void* src0 = nullptr; int C0 = 0;   // first source (channels = row stride of its NHWC tensor)
  const void* src1 = nullptr; int C1 = 0;   // optional second source (skip concat, unet.py:725), never materialised
  int N = 0, Hs = 0, Ws = 0;                // source spatial size
  int mode = CONV_UNIT;
  int ks = 3;
  const float* pro_a = nullptr;             // [N][C0+C1] or null
  const float* pro_b = nullptr;
  int pro_silu = 0;
  const void* w = nullptr;                  // packed by conv_pack_weights
  const void* w_up2 = nullptr;              // optional, mode CONV_UP2 / ks 3: the same filter collapsed to four 2x2 phase filters (conv_pack_weights_up2);
                                            // ConvRoute::w_up2 says whether the launch reads this image instead of w (null: it never does)
  const float* bias = nullptr;              // [Cout]
  int Cout = 0;
  const float* emb = nullptr; int emb_stride = 0;   // per-(n, co) additive term (ResBlock emb_layers)
  const void* res = nullptr; int res_mode = RES_NONE;  // residual NHWC tensor with Cout channels
  void* out = nullptr; int out_mode = OUT_NHWC;
  // optional fused GroupNorm statistics of the OUTPUT (common.h GnPartial): [N][slots][Cout/4][2] fp32, room for gn_slots_cap slots
  // per image; ConvRoute::gn_slots is the number the launch fills (0 = this launch cannot produce them: the caller runs the stats kernel)
  float* gn_stats = nullptr; int gn_slots_cap = 0;
  void* dbg = nullptr;                      // diagnostic builds only (-DCONV_STAMPS): 9 x u64 phase-cycle sums
  const mi355_debug_config* knobs = nullptr; // diagnostic switches (null = defaults)
  uint32_t* err = nullptr;                  // device-visible error word: the persistent kernel ORs 1 into it when a counter wait expires
  // Optional: the GroupNorm (+ SiLU) site that reads this conv's output, applied in the conv's epilogue where the kernel holds whole
  // images x whole groups per wave (conv_small.inc.h): act_out = silu?(GN(out)) in out's layout; out itself only if act_raw; one touch
  // of the next conv's packed weights (warm).  Null: no fusion asked for.  ConvRoute::act_done says whether the launch does it (0: run the pass).
  void* act_out = nullptr; const float* act_gamma = nullptr; const float* act_beta = nullptr;
  const float* act_film = nullptr; int act_film_stride = 0; float act_eps = 1e-5f; int act_silu = 0, act_raw = 1;
  // Where the site is the GroupNorm of a CONCAT consumer (unet.py:650: h = cat([h, hs.pop()])) and its groups are whole inside each
  // source, this conv's output is one source of it: act_out then has act_stride channels per pixel (0 = Cout) of which this conv fills
  // act_coff ..., in groups of act_cpg channels (0 = Cout / 32); act_gamma / act_beta already point at channel act_coff.
  int act_stride = 0, act_coff = 0, act_cpg = 0;
  // A skip connection is read by TWO such sites (the next ResBlock's in_layers norm now, the up path's concat norm later): the second
  // one, same conventions, never FiLM.  ConvRoute::act_done: bit 0 = the first site is applied, bit 1 = the second.
  void* act2_out = nullptr; const float* act2_gamma = nullptr; const float* act2_beta = nullptr;
  int act2_silu = 0, act2_stride = 0, act2_coff = 0, act2_cpg = 0;
  const void* warm = nullptr; uint32_t warm_bytes = 0;
  // Optional (small-level kernel only: conv_route fails where it cannot carry it): out += conv1x1(cat(skip_src0, skip_src1)) - a ResBlock's skip_connection
  // (unet.py:312-317, 351) inside its second conv: centre-tap K chunks of the raw block input at the output resolution.  w then is the image
  // conv_pack_weights_skip made, bias the sum of both biases, res none, src1 none.
  const void* skip_src0 = nullptr; const void* skip_src1 = nullptr; int skip_C0 = 0, skip_C1 = 0;
  // Optional, the network's two edge convs (conv_edge.hip), sampler loops: (i) first conv: the caller's fp32 NCHW tensors x (nchw_c0 channels)
  // and condition (nchw_c1) read directly while the patch is staged - src0's packed NHWC copy (pack_nhwc) is then never made
  // (ConvRoute::reads_nchw says whether the launch does; otherwise it reads src0); (ii) last conv (NCHW fp32 output v): axpy_x += axpy_scale * v
  // instead of storing v - the Euler update x <- x + dt v of the flow-matching sampler (mnist/utils_mnist2.py:118-138) in the epilogue (ConvRoute::axpy)
  const float* nchw0 = nullptr; const float* nchw1 = nullptr; int nchw_c0 = 0, nchw_c1 = 0;
  float* axpy_x = nullptr; float axpy_scale = 0.f;
  int cin_real = 0;                         // > 0: only the first cin_real channels of src0 are non-zero (the network's first conv: in_channels padded to a chunk)
  int wsplit = 0;                           // 1 (bf16x2 precision): w holds [bf16(w) | bf16(w - bf16(w))] along K (twice the chunks): the contraction runs over the
                                            // input channels twice, once against each half - fp32 accumulation of both, activations read (not stored) twice
};

struct ConvGeom {
  int Ho, Wo, BM, BN;
  size_t lds_bytes;
  int grid_m, grid_n;
};
// The kernel conv_launch takes for a description, how it is configured and what it does with the description's optional parts.
enum ConvKernel { CONV_K_IGEMM = 0, CONV_K_1X1, CONV_K_1X1_PP, CONV_K_IN, CONV_K_OUT, CONV_K_PP, CONV_K_WS, CONV_K_SMALL };
struct ConvRoute {
  int kernel = CONV_K_IGEMM;
  ConvGeom geom{};          // the implicit-GEMM tile, or the ping-pong / warp-specialised one (grid_m / grid_n stay the plain launch's: workspace sizing)
  int form = 0;             // 1X1_PP: 0 = 512 x 128, 1 = 256 x 256, 2 = 128 x 256 tiles; OUT: 1 = FIXED; PP: 0 = wide, 1 = narrow, 2 = wide in phase form (up-sampling conv as four 2x2 convs); SMALL: 1 = w8x2
  int BM = 0, GC = 0, ntn = 0;     // 1X1: pixel tile, weight chunks per group, output-channel tiles per workgroup,
  int lvw = 0, lth = 0, G = 0, tiles_x = 0, tiles_y = 0;   //   and its pixel tiling: log2 of the tile's width / height, images per tile
  int n_mt = 0, n_nt = 0;          // 1X1_PP: pixel and channel tiles; 1X1 / SMALL: workgroups along M / N
  int ksplit = 0, sm[10] = {};     // SMALL: waves sharing K; the kernel's sm::Args (conv_small.inc.h), field for field
  size_t lds = 0;                  // dynamic LDS bytes (1X1, OUT, SMALL)
  int gn_slots = 0;         // statistics slots per image the launch fills (0: the caller runs the statistics kernel)
  int act_done = 0;         // bit 0 / 1: the GroupNorm site act_out / act2_out is applied in the epilogue
  int axpy = 0, skip = 0;   // the Euler update replaces the store; the fused 1x1 skip conv is carried
  int reads_nchw = 0;       // the first conv reads the fp32 NCHW tensors nchw0 / nchw1 itself (src0 unused)
  int w_up2 = 0;            // the launch reads ConvDesc::w_up2 (the collapsed weight image of the phase form), not ConvDesc::w
};
// Pure host code (nothing launched or allocated): 0 and *r filled, or < 0 for a description no kernel runs (message set).
int conv_route(const ConvDesc& d, ConvRoute* r);
int conv_launch(const ConvDesc& d, const ConvRoute& r, hipStream_t stream);   // launches r = conv_route(d): 0 or < 0, never "not mine"
int conv_launch(const ConvDesc& d, hipStream_t stream);                       // conv_route, then conv_launch
ConvGeom conv_geometry(const ConvDesc& d);                                    // conv_route(d).geom
// bytes of the packed weight image for a [Cout][Cin][ks][ks] filter
size_t conv_packed_weight_bytes(int dtype, int Cout, int Cin, int ks, int split = 0);
int conv_tile_n(int Cout);
// host-side packing: w_host [Cout][Cin][ks][ks] fp32 (Cin = logical input channels; padded to a chunk)
// split = 1 (bf16 only): [hi | lo] halves along K, hi = bf16(w), lo = bf16(w - hi); the chunk count doubles
void conv_pack_weights(int dtype, const float* w_host, int Cout, int Cin, int ks, void* dst_host, int split = 0);
// a [Cout][Cin][3][3] filter applied behind a nearest-x2 up-sample, collapsed (in fp32) to the four [2][2] filters of the output phases:
// per 128-channel pack tile [phase][chunk][tap 0..3][128 rows][64 B], elements rounded and swizzled as above
size_t conv_packed_weight_bytes_up2(int dtype, int Cout, int Cin);
void conv_pack_weights_up2(int dtype, const float* w_host, int Cout, int Cin, void* dst_host);
// [3x3 filter w3 [Cout][Cin][3][3] | 1x1 filter w1 [Cout][Cskip]] per 128-channel pack tile: the 3x3 tiles, then one tile per skip chunk
size_t conv_packed_weight_bytes_skip(int dtype, int Cout, int Cin, int Cskip);
void conv_pack_weights_skip(int dtype, const float* w3, const float* w1, int Cout, int Cin, int Cskip, void* dst_host);
// The kernel families conv_route asks in turn, one unit each.  X_route: pure host code; 0 = taken (*r filled: kernel, form, geom.BM / BN / lds_bytes, gn_slots,
// act_done, skip, w_up2 and the family's own fields), 1 = not this family (*r untouched), < 0 = error (message set).  X_launch launches such a route: 0 or
// < 0.  conv_pp1.hip: ping-pong 1x1; conv1x1.hip: 1x1 GEMM with a stationary activation tile; conv_edge.hip: the first conv and the last conv (GN + SiLU
// prologue, <= 4 output channels, NCHW fp32).
int pp1_route(const ConvDesc& d, ConvRoute* r);
int pp1_launch(const ConvDesc& d, const ConvRoute& r, hipStream_t stream);
int conv1x1_route(const ConvDesc& d, ConvRoute* r);
int conv1x1_launch(const ConvDesc& d, const ConvRoute& r, hipStream_t stream);
int conv_in_route(const ConvDesc& d, ConvRoute* r);
int conv_in_launch(const ConvDesc& d, const ConvRoute& r, hipStream_t stream);
int conv_out_route(const ConvDesc& d, ConvRoute* r);
int conv_out_launch(const ConvDesc& d, const ConvRoute& r, hipStream_t stream);
// conv_pp.hip (ping-pong 3x3), conv_ws.hip (warp-specialised 3x3), conv_small.hip (8x8 / 4x4 levels): asked behind conv_route's argument checks, with what
// it has worked out by then (ConvPre, conv_kargs.h: the plain tiling and the plain kernel's arguments, which their launches start from)
struct ConvPre;
int pp_route(const ConvDesc& d, const ConvPre& p, ConvRoute* r);
int pp_launch(const ConvDesc& d, const ConvPre& p, const ConvRoute& r, hipStream_t stream);
int ws_route(const ConvDesc& d, const ConvPre& p, ConvRoute* r);
int ws_launch(const ConvDesc& d, const ConvPre& p, const ConvRoute& r, hipStream_t stream);
int small_route(const ConvDesc& d, const ConvPre& p, ConvRoute* r);
int small_launch(const ConvDesc& d, const ConvPre& p, const ConvRoute& r, hipStream_t stream);

// ---- GroupNorm statistics -> per-(n, channel) affine ----------------------------------------------
// a[n,c] = rstd * gamma[c] (* (1 + film_scale)), b[n,c] = beta[c] - mean * rstd * gamma[c] (FiLM folded)
struct GnDesc {
  int dtype;
  const void* src0 = nullptr; int C0 = 0;
  const void* src1 = nullptr; int C1 = 0;
  int N = 0, HW = 0;
  int groups = 32;
  float eps = 1e-5f;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  const float* film = nullptr; int film_stride = 0;  // [N][2C]: scale | shift (use_scale_shift_norm)
  float* a = nullptr;
  float* b = nullptr;
  void* y = nullptr; int y_silu = 0;   // optional: also write silu?(a*x + b), NHWC [N][HW][C0 + C1] (the consumer conv then has no prologue)
  float* mean = nullptr; float* rstd = nullptr;   // optional [N][groups]: kept for the backward pass (reconstruction guidance)
  const void* warm = nullptr; uint32_t warm_bytes = 0;   // optional: packed weights of the conv this pass feeds (common.h l2_warm_issue)
};
int gn_affine_launch(const GnDesc& d, hipStream_t stream);
int gn_affine_form(const GnDesc& d);   // the template form gn_affine_launch takes: NL = 1, 2, 4, 8 (image held in registers) or 0
// The same (a, b) from the partial sums the producing convs left (ConvDesc::gn_stats): no pass over the activation.
struct GnFinDesc {
  const float* stats0 = nullptr; int slots0 = 0, C0 = 0;
  const float* stats1 = nullptr; int slots1 = 0, C1 = 0;
  int N = 0, HW = 0, groups = 32;
  float eps = 1e-5f;
  const float* gamma = nullptr; const float* beta = nullptr;
  const float* film = nullptr; int film_stride = 0;
  float* a = nullptr; float* b = nullptr;
  const void* warm = nullptr; uint32_t warm_bytes = 0;   // as GnDesc::warm
  // the tensors the partials describe (NHWC, C0 / C1 channels, element type dtype): a group whose mean^2 dominates its variance is
  // recomputed from them (gn_stats.hip GN_FIN_RATIO); null: the partial sums are all there is
  int dtype = DT_F32; const void* src0 = nullptr; const void* src1 = nullptr;
};
int gn_finalize_launch(const GnFinDesc& d, hipStream_t stream);
// out = avgpool2x2(silu?(a * in + b)) on NHWC tensors (a, b per (n, c), may be null): the ResBlock(down=True) input path
int affine_pool_launch(int dtype, const void* in, const float* a, const float* b, int silu, void* out, int N, int Hs, int Ws, int C,
                       hipStream_t s);

// ---- attention --------------------------------------------------------------------------------------
// qkv: NHWC [N][T][3*C] with the reference channel order (legacy: per head [q|k|v]; new: [q heads|k heads|v heads])
// out: NHWC [N][T][C]
struct AttnDesc {
  int dtype;
  const void* qkv = nullptr;
  void* out = nullptr;
  int N = 0, T = 0, heads = 0, ch = 0;
  int new_order = 0;
};
int attention_launch(const AttnDesc& d, hipStream_t stream);
// Where head h's channels sit in a [3C] qkv row, either order: q at h * qoff_h, k at koff + h * qoff_h, v at voff + h * qoff_h; and the
// score scale ch^-1/2 (the reference scales q and k by ch^-1/4 each).  Forward and backward launchers alike.
struct AttnChannelOffsets { int qoff_h, koff, voff; float scale2; };
inline AttnChannelOffsets attn_channel_offsets(int new_order, int ch, int C) {
  const float scale2 = 1.0f / sqrtf((float)ch);
  return new_order ? AttnChannelOffsets{ch, C, 2 * C, scale2} : AttnChannelOffsets{3 * ch, ch, 2 * ch, scale2};
}
// GroupNorm-apply -> qkv 1x1 -> attention of one AttentionBlock in one kernel (attn_fused.hip): x NHWC [N][T][C], (a, b) [N][C],
// w / bias = the qkv conv's packed weights (conv_pack_weights, ks 1, Cout 3C) / bias [3C]; out NHWC [N][T][C]
struct AttnFusedDesc {
  int dtype;
  const void* x = nullptr; const float* ga = nullptr; const float* gb = nullptr;
  const void* w = nullptr; const float* bias = nullptr;
  void* out = nullptr;
  int N = 0, T = 0, C = 0, heads = 0, ch = 0, new_order = 0;
  const mi355_debug_config* knobs = nullptr;
  int* form = nullptr;   // optional out, 3 words, written by attn_fused_launch as it decides: {1 per-image | 2 persistent, QB | NCH, 0 | image lanes}
};
bool attn_fused_eligible(int dtype, int T, int C, int heads, int ch, const mi355_debug_config* knobs = nullptr);
int attn_fused_launch(const AttnFusedDesc& d, hipStream_t stream);

// ---- backward (data gradient only: reconstruction guidance, AD/image_diffusion/sampling.py:136-206) --------------------------------
void conv_pack_weights_dgrad(int dtype, const float* w_host, int Cout, int Cin, int ks, int cin_pad, void* dst_host);
size_t conv_packed_weight_bytes_dgrad(int dtype, int Cout, int Cin, int ks, int cin_pad);
struct GnBwdDesc {
  int dtype;
  const void* x0 = nullptr; const void* x1 = nullptr; int C0 = 0, C1 = 0;
  const void* du = nullptr; int du_stride = 0;
  int N = 0, HW = 0, groups = 32, silu = 0;
  const float* a = nullptr; const float* b = nullptr; const float* mean = nullptr; const float* rstd = nullptr;
  void* g0 = nullptr; void* g1 = nullptr; int acc0 = 0, acc1 = 0;
};
int gn_silu_bwd_launch(const GnBwdDesc& d, hipStream_t stream);
enum { GATHER_SAME = 0, GATHER_POOL = 1, GATHER_UP = 2, GATHER_STUFF = 3 };
int grad_gather_launch(int dtype, void* dst, const void* src, int N, int Hd, int Wd, int Cd, int Hs, int Ws, int src_cstride, int src_coff,
                       int mode, int accumulate, float scale, hipStream_t s);
// The data gradient through one conv of the forward plan (input channels cat(src0, src1) -> Cout, ks, mode UNIT / STRIDE2 / UP2): G is the
// gradient of the conv's output, NHWC [N][Hg][Wg][Cg] (Cg = Cout padded to whole chunks), wT the image conv_pack_weights_dgrad made for
// cin_pad = align_up(C0 + C1, 32) output channels.  One bias-free NHWC unit-mode conv of G with wT into du (stride 2: of G zero-stuffed into zbuf
// at the input resolution Hs x Ws; nearest x2: at Hg x Wg = 2 Hs x 2 Ws, its 2x2 block sums are the gradient), then
//   scatter = 1: g0 [N][Hs][Ws][C0] (+)= channels 0 .. C0 of the result, g1 [N][Hs][Ws][C1] (+)= channels C0 .. C0 + C1 (acc0 / acc1: add to
//                what is there; g1 null: one source)
//   scatter = 0: the result stays in scratch for the caller's GroupNorm adjoint (nearest x2: block sums into tmp): ConvDgradOut::dU, rows of
//                dU_stride = cin_pad channels at Hs x Ws, channels >= the forward conv's input channels zero
struct ConvDgradDesc {
  int dtype;
  const void* G = nullptr; int Cg = 0, Hg = 0, Wg = 0;
  const void* wT = nullptr; int cin_pad = 0, ks = 3, mode = CONV_UNIT;
  int N = 0, Hs = 0, Ws = 0;
  void* du = nullptr; void* tmp = nullptr; void* zbuf = nullptr;   // scratch: [N][max(Hs Ws, Hg Wg)][cin_pad], [N][Hs][Ws][cin_pad] (UP2 without scatter), [N][Hs][Ws][Cg] (STRIDE2)
  int scatter = 0;
  void* g0 = nullptr; void* g1 = nullptr; int C0 = 0, C1 = 0, acc0 = 0, acc1 = 0;
  const mi355_debug_config* knobs = nullptr; uint32_t* err = nullptr;   // as ConvDesc's
};
struct ConvDgradOut {
  ConvRoute route;              // what the conv launch was
  const void* dU = nullptr; int dU_stride = 0;
};
int conv_dgrad_launch(const ConvDgradDesc& d, hipStream_t stream, ConvDgradOut* out);
int conv_dgrad_route(const ConvDgradDesc& d, ConvRoute* r);   // the route that launch takes: pure host code, the pointers are not read
struct AttnBwdDesc {
  int dtype;
  const void* qkv = nullptr; const void* a = nullptr; const void* da = nullptr; void* dqkv = nullptr;
  float* L = nullptr; float* D = nullptr;
  int N = 0, T = 0, heads = 0, ch = 0, new_order = 0;
};
int attention_bwd_launch(const AttnBwdDesc& d, hipStream_t stream);
int guidance_seed_launch(const float* x, const float* eps, const float* cond, float c_recip, float c_recipm1, int mode, float pad,
                         int64_t per, float* g_eps, float* g_x, int64_t n, hipStream_t s);
int guidance_update_launch(float* x, const float* g_x, const float* vjp, float scale, int apply, float* update, int64_t n, hipStream_t s);
// the seed of the low-resolution consistency term mean((D(x0) - y_low)^2), D the bilinear reduction to hl x wl (H % hl == 0, W % wl == 0, else -4
// before a launch): resid [B,C,hl,wl] scratch, loss [B] or null; two launches, three with loss
int lowres_seed_launch(const float* x, const float* eps, const float* y_low, float c_recip, float c_recipm1, int B, int C, int H, int W, int hl,
                       int wl, float* resid, float* g_eps, float* g_x, float* loss, hipStream_t s);
// out[n][c][hw] (NCHW fp32, c < count) = in[n][hw][c0 + c] (NHWC T, row stride `stride`)
int unpack_channels_launch(int dtype, const void* in, int N, int HW, int stride, int c0, int count, float* out, hipStream_t s);

// ---- box calibration probe (box_probe.hip: frozen) ------------------------------------------------------------------------------
int64_t box_probe_workspace_bytes();
double box_probe_flops();
int box_probe_run(int reps, void* workspace, int64_t workspace_bytes, hipStream_t s, float* us_per_launch, float* clock_mhz);
// memory side (box_probe_hbm.hip: frozen): one launch copies 512 MiB to another 512 MiB
int64_t box_probe_hbm_workspace_bytes();
double box_probe_hbm_bytes();
int box_probe_hbm_run(int reps, void* workspace, int64_t workspace_bytes, hipStream_t s, float* us_per_launch);

// ---- small fp32 ops -----------------------------------------------------------------------------------
int timestep_embedding_launch(const float* t, int B, int dim, float max_period, float* out, hipStream_t s);
// out[b][j] = bias[j] + sum_k act(in[b][k]) * Wt[k][j]   (Wt = transposed weights, [K][J]); act: 0 none, 1 silu(in)
// out_act: 0 none, 1 silu(out)
int linear_launch(const float* in, const float* Wt, const float* bias, float* out, int B, int K, int J, int in_act,
                  int out_act, hipStream_t s);
int linear_form(int B, int K);   // the kernel linear_launch takes: 0 = linear_kernel (8-row slabs in LDS), 1 = linear_small_kernel (K split over four waves)
// Class-conditional emb_layers (R rows): out[r][j] = bias[j] + sum_k silu(h[r / h_div][k] + lemb[lab(r)][k]) * Wt[k][j], lab(r) = labels ?
// labels[r] : r % n_classes.  A label outside [0, n_classes) adds a zero row and stores 2 into the error word `err` (if not null).
int label_emb_linear_launch(const float* h, int h_div, const float* lemb, const int32_t* labels, int n_classes, const float* Wt,
                            const float* bias, float* out, int R, int K, int J, uint32_t* err, hipStream_t s);
int label_emb_linear_form(int K);   // rows per slab of the template form label_emb_linear_launch takes: 16 (K <= 1024) or 8
// out[b] = table[labels[b]] (rows of J floats, J % 4 == 0); a label outside [0, n_classes) gives a zero row and stores 2 into `err`
int emb_gather_launch(const float* table, const int32_t* labels, int n_classes, float* out, int B, int J, uint32_t* err, hipStream_t s);

// NCHW fp32 (x | cond) -> NHWC T with channels padded to Cpad (zero fill)
int pack_nhwc_launch(int dtype, const float* x, int Cx, const float* cond, int Cc, int N, int HW, int Cpad, void* out,
                     hipStream_t s);
// NHWC T [N][HW][C] -> NCHW fp32
int unpack_nchw_launch(int dtype, const void* in, int N, int HW, int C, float* out, hipStream_t s);
// plain resampling of NHWC tensors (conv_resample=False paths): mode CONV_UP2 / CONV_POOL2
int resample_launch(int dtype, const void* in, void* out, int N, int Hs, int Ws, int C, int mode, hipStream_t s);

// elementwise sampler steps (steps.hip)
int euler_step_launch(float* x, const float* v, float dt, int64_t n, hipStream_t s);
int sde_euler_step_launch(float* x, const float* a, const float* b, float ca, float cb, float dt, const float* g, float g_s, const float* dW,
                          int use_philox, uint64_t seed, uint64_t offset, float* out, float w, int64_t n, hipStream_t s);
// What a DDPM net's output stands for (mi355_ddpm_prediction::kind): the noise eps, the data x0 itself, or v = sa eps - sb x0 (Salimans & Ho 2022).
// Every consumer forms the unclipped data prediction x0_pre of the kind - eps: c_recip x - c_recipm1 out; x0: out (x is not read for it); v: sa x - sb out,
// sa = sqrt_alphas_cumprod, sb = sqrt_one_minus_alphas_cumprod of the step - and goes on from it as it always did.
enum { PRED_EPS = 0, PRED_X0 = 1, PRED_V = 2 };
// per, eps_stride (0, 0: contiguous): eps of image b of `per` elements is read at eps + b * eps_stride (PredictorStep::eps_stride); pred, sa, sb: PRED_*
int corrector_step_launch(float* x, const float* eps, const float* z, float c_recip, float c_recipm1, float rsm1, float dt,
                          float delta, int use_philox, uint64_t seed, uint64_t offset, int64_t n, hipStream_t s, int64_t per = 0, int64_t eps_stride = 0,
                          int pred = PRED_EPS, float sa = 0.f, float sb = 0.f);
int renoise_step_launch(float* x, const float* z, float a, float b, int use_philox, uint64_t seed, uint64_t offset, int64_t n, hipStream_t s);
// The predictor steps of the DDPM loops: ONE descriptor, ONE launcher.  Every kind forms the data prediction x0_hat = clip(c_recip x - c_recipm1 eps)
// and moves x from it:
//   STEP_ANCESTRAL  a, b = posterior_mean_coef1, coef2: x <- a x0_hat + b x + sigma z
//   STEP_DDIM       a = acp_prev:                       x <- sqrt(a) x0_hat + sqrt(1 - a) e2, e2 the eps that x0_hat stands for
//   STEP_DDIM_ETA   a = acp_prev, sigma finite >= 0:    the same with sqrt(max(1 - a - sigma^2, 0)) and + sigma z (no noise given: no noise term)
//   STEP_DPMPP      a, b, c = cx, c0, c1:               x <- a x + b x0_hat + c hist; hist <- x0_hat (hist: not read when c == 0, not written when null)
//   STEP_ANCESTRAL_LV  a, b as STEP_ANCESTRAL; min_log, max_log: x <- a x0_hat + b x + exp(0.5 logvar) z, logvar = frac max_log + (1 - frac) min_log,
//                   frac = (v + 1) / 2, v read at eps + per under eps_stride (>= 2 per): the learned variance range of improved DDPM; no shaping rows
// eps_stride (0 = per, the contiguous read): element r of image b is read at eps[b * eps_stride + r] - the eps channels of a [B, 2C, H, W] network
// output with per = C H W and eps_stride = 2 per; in the guided forms the unconditional half starts at B * eps_stride.  Not with shaping rows.
// Noise (the kinds with a z term): z injected, or Philox at (seed, offset), offset a multiple of 4, indexed by the element of the n-element state.
// guide.on: eps [2n] = conditional | unconditional evaluation, combined as eps_u + w (eps_c - eps_u) with w, or w_dev[image] over images of `per`
// elements; x [2n] is the duplicated state (first half read, both halves written).  shape (null: the static clip to [-1, 1]): rows (f, s) per image of
// `per` elements, filled by x0_shape_stats_launch: eps is scaled by f, x0_hat = clip(x0, -s, s) / s.  Refusals are prefixed ddpm_step, ddpm_cfg_step,
// ddim_step, ... dpmpp_cfg_step after the kind and guide.on.
enum { STEP_ANCESTRAL = 0, STEP_DDIM = 1, STEP_DDIM_ETA = 2, STEP_DPMPP = 3, STEP_ANCESTRAL_LV = 4 };
struct StepGuide { bool on = false; float w = 0.f; const float* w_dev = nullptr; };
struct PredictorStep {
  int kind = STEP_ANCESTRAL;   // a STEP_* value (mi355_x0_shaped_step, which takes it from its caller, checks the range)
  float* x = nullptr; const float* eps = nullptr; const float* z = nullptr; float* hist = nullptr;
  float c_recip = 0.f, c_recipm1 = 0.f;
  float a = 0.f, b = 0.f, c = 0.f, sigma = 0.f;
  int use_philox = 0; uint64_t seed = 0, offset = 0;
  StepGuide guide;
  int64_t per = 0; const float* shape = nullptr; int64_t n = 0;
  int64_t eps_stride = 0;
  float min_log = 0.f, max_log = 0.f;
  int pred = PRED_EPS; float sa = 0.f, sb = 0.f;   // what `eps` holds (PRED_*); sa, sb are read by PRED_V alone
};
int predictor_step_launch(const PredictorStep& p, hipStream_t s);
// The null-space (DDNM) predictor step (nullspace.hip; the arithmetic: its file comment and include/mi355_sampler.h): the data prediction of the state
// [batch, channels, h, w] is rectified against the measurement y of `op` with the step's lam, then the state moves from it by form 0 (ancestral: a, b =
// posterior_mean_coef1, coef2) or form 1 (DDIM(eta): a = acp_prev).  out: the network output, image b at out + b * out_stride (0: contiguous); pred, sa,
// sb: PRED_*.  Noise as the predictor steps'.  One launch; check_nullspace_op holds the refusals of an operator against an h x w state, prefixed by `who`.
struct NullspaceStep {
  const mi355_nullspace_op* op = nullptr;
  int form = 0;
  float* x = nullptr; const float* out = nullptr; int64_t out_stride = 0; const float* y = nullptr; const float* z = nullptr;
  int batch = 0, channels = 0, h = 0, w = 0;
  float c_recip = 0.f, c_recipm1 = 0.f, a = 0.f, b = 0.f, lam = 0.f, sigma = 0.f;
  int use_philox = 0; uint64_t seed = 0, offset = 0;
  int pred = PRED_EPS; float sa = 0.f, sb = 0.f;
};
int check_nullspace_op(const char* who, const mi355_nullspace_op* op, int h, int w);
int nullspace_step_launch(const NullspaceStep& p, hipStream_t s);
// out [planes, h_low, w_low] = the block means of in [planes, h, w]: A of operator kind 1, in the step's summation order (the same bits)
int block_mean_launch(const float* in, float* out, int64_t planes, int h, int w, int h_low, int w_low, hipStream_t s);
// The statistics behind `shape`, one workgroup per image (and detail [B, 4] = sigma_c, sigma_g, s_raw, 0 when not null); check_x0_shaping holds the
// refusals of a mi355_x0_shaping (null: none), each prefixed by `who`.
int check_x0_shaping(const char* who, const mi355_x0_shaping* sh, int guided);
int x0_shape_stats_launch(const float* x, const float* eps, const StepGuide& g, float c_recip, float c_recipm1, const mi355_x0_shaping* sh, float* shape,
                          float* detail, int batch, int64_t per, hipStream_t s, int pred = PRED_EPS, float sa = 0.f, float sb = 0.f);
int replace_mask_launch(float* x, const float* cond, const float* z, float pad, int noisy, float sa, float sb,
                        int use_philox, uint64_t seed, uint64_t offset, int64_t n, hipStream_t s);
int clip_launch(float* x, float lo, float hi, int64_t n, hipStream_t s);
// q(x_k | x_0) out of place (steps.hip): out = a x0 + b z, products and sum each rounded; noise as the ancestral step
int q_sample_launch(float* out, const float* x0, const float* z, float a, float b, int use_philox, uint64_t seed, uint64_t offset, int64_t n,
                    hipStream_t s);
// The variational bound of a DDPM net (vlb.hip; the formulas: include/mi355_sampler.h, mi355_ddpm_vlb).  One step's three per-image numbers
// dst[b * dst_stride + 0..2] = { vb, xstart_mse, mse } from x0, x_k [batch][per], the network output out (eps of image b at out + b * out_stride, v
// behind it at + per, read iff learned) and the step's draw (z [batch][per], or Philox at (seed, offset) regenerated); fp64 per element, sums in a
// fixed order, each number rounded to fp32 once.  k_is_zero: the discretised decoder (cdf 0: erfc, 1: the tanh approximation) in place of the KL.
struct VlbStep {
  float c_recip = 0.f, c_recipm1 = 0.f, coef1 = 0.f, coef2 = 0.f;   // the chain tables at step k
  float true_log = 0.f;                                             // log-variance of q(x_{k-1} | x_k, x_0)
  float model_log = 0.f;                                            // the model's, fixed (read iff !learned)
  float min_log = 0.f, max_log = 0.f;                               // the learned range (read iff learned)
  int k_is_zero = 0, learned = 0, cdf = 0, clip = 0;
  int pred = PRED_EPS; float sa = 0.f, sb = 0.f;                     // what `out` holds (PRED_*): x0_hat from x0_pre of the kind, mse against the kind's training
                                                                    // target (z; x0; sa z - sb x0); sa, sb = sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod at k
};
int vlb_terms_launch(const float* x0, const float* xk, const float* out, int64_t out_stride, const float* z, int use_philox, uint64_t seed,
                     uint64_t offset, const VlbStep& st, float* dst, int64_t dst_stride, int batch, int64_t per, hipStream_t s);
// summary[b * 2] = prior_bpd of image b; with terms (vb of step k of image b at terms[b * terms_stride + 3 k], k < K) also summary[b * 2 + 1] =
// the fp64 sum of the K vb values and the rounded prior, rounded once
int vlb_prior_launch(const float* x0, float sa_last, float sb_last, const float* terms, int64_t terms_stride, int K, float* summary, int batch,
                     int64_t per, hipStream_t s);
int mse_per_sample_launch(const float* a, const float* b, float* out, int batch, int64_t per, hipStream_t s);
// out[b] = ||cur_b - prev_b||^2 / ||prev_b||^2, then prev <- cur; cur, prev [batch][per] of the internal dtype's element type (steps.hip)
int feature_drift_launch(int dtype, const void* cur, void* prev, int batch, int64_t per, float* out, hipStream_t s);
int lincomb_per_sample_launch(float* out, const float* x, const float* y, const float* a, const float* b, int batch, int64_t per,
                              hipStream_t s);
// per-sample { mse, data_range, psnr, ssim } of x against ref, one workgroup per sample (metrics.hip); taps_host NULL = uniform window
int image_metrics_launch(const float* x, const float* ref, float* out, int batch, int channels, int h, int w, float data_range,
                         const float* taps_host, int win, float cov_norm, float k1, float k2, hipStream_t s);
int ema_update_launch(float* target, const float* source, float decay, float one_minus_decay, int64_t n, hipStream_t s);
int quantize_u8_launch(const float* x, uint8_t* out, int64_t n, hipStream_t s);
int to_unit_range_launch(const float* x, float* out, int64_t n, hipStream_t s);
int randn_launch(float* out, uint64_t seed, uint64_t offset, int64_t n, hipStream_t s);
int fill_launch(float* x, float v, int64_t n, hipStream_t s);
// condition builders (steps.hip): bilinear resize of NCHW fp32 planes (align_corners = False), square-patch painting of a batch
int resize_bilinear_launch(const float* in, float* out, int64_t planes, int Hi, int Wi, int Ho, int Wo, hipStream_t s);
int paint_patch_launch(const float* img, const int* top, const int* left, int patch, float pad, int outpaint, float* out, int N, int C,
                       int H, int W, hipStream_t s);
int groupnorm_nchw_launch(const float* x, const float* gamma, const float* beta, float* y, int N, int C, int HW, int groups,
                          float eps, int silu, hipStream_t s);

// tiled sampling (tile.hip): the geometry of a mi355_tile_plan over a net of frame S (tile_geom holds every refusal that needs no handle, each
// prefixed by `who`), the copy of a canvas [B, C, Hc, Wc] into its windows [B * nW, C, S, S] (labels: [B] -> [B * nW]), and the weighted average of
// window predictions back onto the canvas (vbar, and x <- x + dt * vbar where euler_x is given)
struct TileGeom { int S, Hc, Wc, sy, sx, ny, nx, nW, weight; };
int tile_geom(int image_size, const mi355_tile_plan* plan, TileGeom* g, const char* who);
inline int tile_origin(int i, int s, int L, int S) { return i * s < L - S ? i * s : L - S; }
int tile_gather_launch(const float* canvas, float* windows, int B, int C, const TileGeom& g, hipStream_t s);
int tile_labels_launch(const int32_t* labels, int32_t* out, int B, int nW, hipStream_t s);
int tile_blend_launch(const float* windows, float* vbar, float* euler_x, float dt, int B, int C, const TileGeom& g, hipStream_t s);

// adaptive RK45 helpers (ode.hip)
int rk_combine_launch(float* out, const float* y0, const float* const* k, const float* c, int nk, int64_t n, hipStream_t s);
// one stage of a fixed-step explicit RK sampler: out = y0 + sum_j c[j] * k[j] (1 <= nk <= 4; out may be y0), the result also to copy_out and,
// quantised as quantize_u8_launch does, to u8_out (either may be null)
int rk_stage_launch(float* out, const float* y0, const float* const* k, const float* c, int nk, int64_t n, float* copy_out, uint8_t* u8_out,
                    hipStream_t s);
// rk_stage over guided derivatives: k[j] [2n] = conditional | unconditional evaluation, g_j = ku + w * (kc - ku) (w_dev: one scale per image of
// `per` elements), out = y0 + sum_j c[j] * g_j (y0 may be null); dup: also to out + n
int cfg_stage_launch(float* out, const float* y0, const float* const* k, const float* c, int nk, int64_t n, float w, const float* w_dev, int64_t per,
                     int dup, float* copy_out, uint8_t* u8_out, hipStream_t s);
int rk_sqnorm_launch(const float* a, const float* sub, const float* b, const float* b2, float atol, float rtol, int64_t n, double* out,
                     hipStream_t s);
int rk_interp_launch(float* out, const float* y0, const float* y1, const float* ym, const float* f0, const float* f1, float dt, float x,
                     int64_t n, hipStream_t s);
