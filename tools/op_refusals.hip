// Host-only record of what the single-op test harness of libmi355_sampler.so (csrc/test_ops.hip) answers before it touches a device: for every op
// the return code and mi355_last_error() text of calls with ONE fault each, and for mi355_conv2d_fwd and mi355_conv2d_vjp the route words of
// their dry route query (host code only) over a small table of shapes, modes, kernel sizes, element types and switches.  Pointers are made up and
// never read; nothing is launched and no device is needed.  Every faulted call must be refused before the op's first HIP call, in words that name
// the fault: a case that returns 0 or MI355_ERR_HIP, or that is refused in other words, fails the program.  No call is made that the host checks
// would accept (the route queries apart, which launch nothing), and the program must not be run where a device is present (it refuses to start
// there): an accepted call would launch on made-up addresses.  Build it with the host code under a sanitizer (make -C <package>/csrc op_refusals)
// and run it: it must exit 0 with no report.  It reads include/mi355_sampler.h alone, so the same source builds against an earlier commit: two builds
// of the library whose harness checks the same things in the same words and routes alike print the same bytes.  Keep the output of the build before
// a change of the harness and compare.  It is a program of its own: never load it into Python.
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../include/mi355_sampler.h"

namespace {

template <class T> T* fake(int k) { return reinterpret_cast<T*>(uintptr_t(k) << 40); }   // made-up addresses, never dereferenced
float* const X = fake<float>(3); float* const X1 = fake<float>(4); float* const Wt = fake<float>(5); float* const Bs = fake<float>(6);
float* const Y = fake<float>(7); float* const P = fake<float>(8); float* const Q = fake<float>(9); float* const G0 = fake<float>(10);
float* const G1 = fake<float>(11); void* const WS = fake<void>(2); int32_t* const LAB = fake<int32_t>(12);
constexpr int64_t BIG = int64_t(1) << 50, SHORT = 4096;   // a workspace no op outgrows; one every op outgrows
constexpr int F32 = MI355_F32, BF = MI355_BF16, X2 = MI355_BF16X2, F16 = MI355_F16, BAD = 7;

mi355_debug_config knobs() { mi355_debug_config k; mi355_debug_defaults(&k); return k; }
mi355_debug_config fused_attention() { mi355_debug_config k = knobs(); k.attn_fused = 1; return k; }

// mi355_conv2d's arguments at values the op accepts (a plain 3x3 conv 64 -> 64 on 8x8 images, bf16); a case changes one thing
struct Conv {
  const float* x = X; const float* x1 = nullptr; int cin1 = 0; const float* w = Wt; float* y = Y; int batch = 2, cin = 64, h = 8, wd = 8, cout = 64, k = 3, stride = 1,
      resample = 0; const float* emb = nullptr; const float* res = nullptr; int res_mode = 1, dtype = BF; void* ws = WS; int64_t ws_bytes = BIG;
  int call() const { return mi355_conv2d(x, x1, cin1, w, Bs, y, batch, cin, h, wd, cout, k, stride, resample, nullptr, nullptr, 0, emb, res, res_mode, dtype, nullptr, ws, ws_bytes, nullptr); }
  int call_ex(mi355_conv_extras* ex) const {
    return mi355_conv2d_ex(x, x1, cin1, w, Bs, y, batch, cin, h, wd, cout, k, stride, resample, nullptr, nullptr, 0, emb, res, res_mode, dtype, nullptr, ws, ws_bytes, nullptr, ex);
  }
};
template <class F> int conv(F change) { Conv c; change(c); return c.call(); }
template <class F> int conv_ex(F change) { Conv c; change(c); mi355_conv_extras ex{}; return c.call_ex(&ex); }

// mi355_conv2d_fwd's, the same conv; dry: the route query (no workspace, no pointer read)
struct Fwd {
  const float* x = X; const float* x1 = nullptr; int cin1 = 0; const float* w = Wt; float* y = Y; int batch = 2, cin = 64, h = 8, wd = 8, cout = 64, k = 3, stride = 1,
      resample = 0; const float* pro_a = nullptr; const float* pro_b = nullptr; int pro_silu = 0; const float* emb = nullptr; const float* res = nullptr;
  int res_mode = 1, flags = 0; float* axpy = nullptr; int dtype = BF; const mi355_debug_config* debug = nullptr; int32_t* route = nullptr; void* ws = WS;
  int64_t ws_bytes = BIG;
  int call() const {
    return mi355_conv2d_fwd(x, x1, cin1, w, Bs, y, batch, cin, h, wd, cout, k, stride, resample, pro_a, pro_b, pro_silu, emb, res, res_mode, flags, axpy, 0.5f, dtype,
                            debug, route, ws, ws_bytes, nullptr);
  }
};
template <class F> int fwd(F change) { Fwd c; change(c); return c.call(); }

// mi355_conv2d_vjp's: the data gradient of a plain 3x3 conv 64 -> 64 on 8x8 images into g0
struct Vjp {
  const float* w = Wt; const float* go = X; float* g0 = G0; float* g1 = nullptr; float* raw = nullptr; int acc0 = 0, acc1 = 0, batch = 2, cout = 64, cin = 64, c0 = 64,
      c1 = 0, h = 8, wd = 8, k = 3, mode = 0, gch = 64, dtype = BF; const mi355_debug_config* debug = nullptr; int32_t* route = nullptr; void* ws = WS; int64_t ws_bytes = BIG;
  int call() const { return mi355_conv2d_vjp(w, go, g0, g1, raw, acc0, acc1, batch, cout, cin, c0, c1, h, wd, k, mode, gch, dtype, debug, route, ws, ws_bytes, nullptr); }
};
template <class F> int vjp(F change) { Vjp c; change(c); return c.call(); }

int gn_affine(const float* x, const float* x1, int c1, float* mean, float* rstd, int batch, int dtype) {
  return mi355_gn_affine(x, x1, P, Q, nullptr, 1e-5f, G0, G1, mean, rstd, nullptr, 0, nullptr, batch, 64, c1, 64, dtype, nullptr);
}
int conv_gn(const float* x1, int cout1, int stride, int resample, int cout0, int dtype) {
  static int32_t words[6];
  return mi355_conv2d_gn(X, Wt, Bs, Y, 64, cout0, x1, x1 ? Wt : nullptr, nullptr, x1 ? Y : nullptr, x1 ? 64 : 0, cout1, 2, 8, 8, 3, stride, resample, P, Q, nullptr, 1e-5f,
                         G0, G1, dtype, nullptr, words, nullptr);
}
int gn_vjp(const float* x1, float* g1, int c1, int du_stride, int batch, int dtype) {
  return mi355_gn_silu_vjp(X, x1, P, Q, nullptr, 1e-5f, 1, Y, du_stride, G0, g1, 0, 0, batch, 64, c1, 64, dtype, nullptr);
}
int gather(int hs, int ws, int src_channels, int coff, int mode, int dtype, const float* src = X) {
  return mi355_grad_gather(src, Y, 2, 64, 8, 8, hs, ws, src_channels, coff, mode, 0, 1.f, dtype, nullptr);
}
int attn(const float* qkv, int dtype, int64_t ws_bytes) { return mi355_qkv_attention(qkv, Y, 2, 2, 64, 64, 0, dtype, WS, ws_bytes, nullptr); }
int attn_vjp(const float* qkv, int batch, int dtype, int64_t ws_bytes) { return mi355_qkv_attention_vjp(qkv, X1, Y, batch, 2, 64, 64, 0, dtype, WS, ws_bytes, nullptr); }
int attn_block(const float* x, int batch, int length, int dtype, int64_t ws_bytes) {
  static const mi355_debug_config k = fused_attention();
  int32_t form[3];
  return mi355_attn_block_fused(x, P, Q, Wt, Bs, Y, batch, 128, length, 2, 0, dtype, &k, form, WS, ws_bytes, nullptr);
}

// One line per case.  expect: what the refusal must say of the fault (alternatives separated by |); a refusal in other words was made for another
// reason, so the fault was not the call's only one.
struct Case { const char* op; const char* what; const char* expect; int (*call)(); };
const Case cases[] = {
    // ---- mi355_conv2d / mi355_conv2d_ex (first HIP call: zeroing the error word, after the workspace check; the shapes are not phase-eligible) ----
    {"conv2d", "null x", "null argument", [] { return conv([](Conv& c) { c.x = nullptr; }); }},
    {"conv2d", "null workspace", "null argument", [] { return conv([](Conv& c) { c.ws = nullptr; }); }},
    {"conv2d", "dtype 7", "dtype", [] { return conv([](Conv& c) { c.dtype = BAD; }); }},
    {"conv2d", "stride 3", "stride must be", [] { return conv([](Conv& c) { c.stride = 3; }); }},
    {"conv2d", "stride 2 with nearest x2", "combined", [] { return conv([](Conv& c) { c.stride = 2; c.resample = 2; }); }},
    {"conv2d", "x1 without cin1", "go together", [] { return conv([](Conv& c) { c.x1 = X1; }); }},
    {"conv2d", "cin1 without x1", "go together", [] { return conv([](Conv& c) { c.cin1 = 64; }); }},
    {"conv2d", "res_mode 3", "res_mode", [] { return conv([](Conv& c) { c.res = P; c.res_mode = 3; }); }},
    {"conv2d", "two sources, 48 + 32 bf16 channels", "two-source", [] { return conv([](Conv& c) { c.cin = 48; c.x1 = X1; c.cin1 = 32; }); }},
    {"conv2d", "two sources, 24 + 16 fp32 channels", "two-source", [] { return conv([](Conv& c) { c.dtype = F32; c.cin = 24; c.x1 = X1; c.cin1 = 16; }); }},
    {"conv2d", "pooling over a concat", "pooling", [] { return conv([](Conv& c) { c.resample = 3; c.x1 = X1; c.cin1 = 64; }); }},
    {"conv2d", "emb with 3 output channels", "NHWC", [] { return conv([](Conv& c) { c.cout = 3; c.emb = P; }); }},
    {"conv2d", "short workspace", "workspace too small", [] { return conv([](Conv& c) { c.ws_bytes = SHORT; }); }},
    {"conv2d", "short workspace, stride 2, bf16x2", "workspace too small", [] { return conv([](Conv& c) { c.stride = 2; c.dtype = X2; c.ws_bytes = SHORT; }); }},
    {"conv2d_ex", "null extras", "null extras", [] { Conv c; return c.call_ex(nullptr); }},
    {"conv2d_ex", "null w_host", "null argument", [] { return conv_ex([](Conv& c) { c.w = nullptr; }); }},
    {"conv2d_ex", "dtype 7", "dtype", [] { return conv_ex([](Conv& c) { c.dtype = BAD; }); }},
    {"conv2d_ex", "stride 0", "stride must be", [] { return conv_ex([](Conv& c) { c.stride = 0; }); }},
    {"conv2d_ex", "res_mode 0", "res_mode", [] { return conv_ex([](Conv& c) { c.res = P; c.res_mode = 0; }); }},
    {"conv2d_ex", "short workspace", "workspace too small", [] { return conv_ex([](Conv& c) { c.ws_bytes = SHORT; }); }},
    // ---- the attention ops (first HIP call: the pack launch, after the workspace check) ----
    {"qkv_attention", "null qkv", "null argument", [] { return attn(nullptr, BF, BIG); }},
    {"qkv_attention", "dtype MI355_BF16X2", "dtype", [] { return attn(X, X2, BIG); }},
    {"qkv_attention", "dtype 7", "dtype", [] { return attn(X, BAD, BIG); }},
    {"qkv_attention", "short workspace", "workspace too small", [] { return attn(X, BF, SHORT); }},
    {"qkv_attention_vjp", "null qkv", "null argument", [] { return attn_vjp(nullptr, 2, BF, BIG); }},
    {"qkv_attention_vjp", "dtype MI355_F16", "MI355_F32 or MI355_BF16", [] { return attn_vjp(X, 2, F16, BIG); }},
    {"qkv_attention_vjp", "dtype MI355_BF16X2", "MI355_F32 or MI355_BF16", [] { return attn_vjp(X, 2, X2, BIG); }},
    {"qkv_attention_vjp", "batch 0", "bad sizes", [] { return attn_vjp(X, 0, BF, BIG); }},
    {"qkv_attention_vjp", "short workspace", "workspace too small", [] { return attn_vjp(X, 2, F32, SHORT); }},
    {"attn_block_fused", "null x", "null argument", [] { return attn_block(nullptr, 2, 256, BF, BIG); }},
    {"attn_block_fused", "dtype MI355_BF16X2", "dtype must be", [] { return attn_block(X, 2, 256, X2, BIG); }},
    {"attn_block_fused", "dtype 7", "dtype must be", [] { return attn_block(X, 2, 256, BAD, BIG); }},
    {"attn_block_fused", "batch 0", "bad sizes", [] { return attn_block(X, 0, 256, BF, BIG); }},
    {"attn_block_fused", "100 tokens", "not supported by the fused kernel", [] { return attn_block(X, 2, 100, BF, BIG); }},
    {"attn_block_fused", "short workspace", "workspace too small", [] { return attn_block(X, 2, 256, BF, SHORT); }},
    // ---- the GroupNorm ops (first HIP call: the op's own allocation, after every argument check) ----
    {"gn_affine", "null x", "bad argument", [] { return gn_affine(nullptr, nullptr, 0, P, Q, 2, BF); }},
    {"gn_affine", "batch 0", "bad argument", [] { return gn_affine(X, nullptr, 0, P, Q, 0, BF); }},
    {"gn_affine", "x1 without c1", "go together", [] { return gn_affine(X, X1, 0, P, Q, 2, BF); }},
    {"gn_affine", "mean without rstd", "go together", [] { return gn_affine(X, nullptr, 0, P, nullptr, 2, BF); }},
    {"gn_affine", "dtype MI355_BF16X2", "dtype must be", [] { return gn_affine(X, nullptr, 0, P, Q, 2, X2); }},
    {"gn_affine", "dtype 7", "dtype must be", [] { return gn_affine(X, nullptr, 0, P, Q, 2, BAD); }},
    {"conv2d_gn", "null info", "bad argument", [] { return mi355_conv2d_gn(X, Wt, Bs, Y, 64, 64, nullptr, nullptr, nullptr, nullptr, 0, 0, 2, 8, 8, 3, 1, 0, P, Q, nullptr, 1e-5f, G0, G1, BF, nullptr, nullptr, nullptr); }},
    {"conv2d_gn", "x1 without cout1", "second producer", [] { return conv_gn(X1, 0, 1, 0, 64, BF); }},
    {"conv2d_gn", "stride 3", "stride 1 or 2", [] { return conv_gn(nullptr, 0, 3, 0, 64, BF); }},
    {"conv2d_gn", "resample 3", "resample 0 or 2", [] { return conv_gn(nullptr, 0, 1, 3, 64, BF); }},
    {"conv2d_gn", "stride 2 with nearest x2", "stride 1 or 2", [] { return conv_gn(nullptr, 0, 2, 2, 64, BF); }},
    {"conv2d_gn", "dtype MI355_BF16X2", "dtype must be", [] { return conv_gn(nullptr, 0, 1, 0, 64, X2); }},
    {"conv2d_gn", "48 output channels", "cout % 32", [] { return conv_gn(nullptr, 0, 1, 0, 48, BF); }},
    {"affine_pool", "a without b", "bad argument", [] { return mi355_affine_pool(X, P, nullptr, 0, Y, 2, 64, 8, 8, BF, nullptr); }},
    {"affine_pool", "channels 0", "bad argument", [] { return mi355_affine_pool(X, nullptr, nullptr, 0, Y, 2, 0, 8, 8, BF, nullptr); }},
    {"affine_pool", "dtype MI355_BF16X2", "dtype must be", [] { return mi355_affine_pool(X, nullptr, nullptr, 0, Y, 2, 64, 8, 8, X2, nullptr); }},
    {"gn_silu_vjp", "batch 0", "bad argument", [] { return gn_vjp(nullptr, nullptr, 0, 64, 0, BF); }},
    {"gn_silu_vjp", "dtype MI355_F16", "MI355_F32 or MI355_BF16", [] { return gn_vjp(nullptr, nullptr, 0, 64, 2, F16); }},
    {"gn_silu_vjp", "dtype MI355_BF16X2", "MI355_F32 or MI355_BF16", [] { return gn_vjp(nullptr, nullptr, 0, 64, 2, X2); }},
    {"gn_silu_vjp", "x1 without g1", "go together", [] { return gn_vjp(X1, nullptr, 32, 96, 2, BF); }},
    {"gn_silu_vjp", "c1 without x1", "go together", [] { return gn_vjp(nullptr, nullptr, 32, 96, 2, BF); }},
    {"gn_silu_vjp", "du_stride 64 for 96 channels", "du_stride", [] { return gn_vjp(X1, G1, 32, 64, 2, BF); }},
    {"grad_gather", "null src", "bad argument", [] { return gather(8, 8, 64, 0, 0, BF, nullptr); }},
    {"grad_gather", "dtype MI355_F16", "MI355_F32 or MI355_BF16", [] { return gather(8, 8, 64, 0, 0, F16); }},
    {"grad_gather", "dtype 7", "MI355_F32 or MI355_BF16", [] { return gather(8, 8, 64, 0, 0, BAD); }},
    {"grad_gather", "channels 32 .. 96 of 64", "inside the source", [] { return gather(8, 8, 64, 32, 0, BF); }},
    {"grad_gather", "identity from 16x16", "does not match the mode", [] { return gather(16, 16, 64, 0, 0, BF); }},
    {"grad_gather", "2x2 blocks of 8x8", "does not match the mode", [] { return gather(8, 8, 64, 0, 1, BF); }},
    {"grad_gather", "half resolution 3x4", "does not match the mode", [] { return gather(3, 4, 64, 0, 2, F32); }},
    {"grad_gather", "mode 7", "does not match the mode", [] { return gather(8, 8, 64, 0, 7, BF); }},
    // ---- mi355_conv2d_vjp (first HIP call: zeroing the error word, after the workspace check) ----
    {"conv2d_vjp", "dtype MI355_F16", "MI355_F32 or MI355_BF16", [] { return vjp([](Vjp& c) { c.dtype = F16; }); }},
    {"conv2d_vjp", "dtype MI355_BF16X2", "MI355_F32 or MI355_BF16", [] { return vjp([](Vjp& c) { c.dtype = X2; }); }},
    {"conv2d_vjp", "null w_host", "null argument", [] { return vjp([](Vjp& c) { c.w = nullptr; }); }},
    {"conv2d_vjp", "null workspace of 1 byte", "null argument", [] { return vjp([](Vjp& c) { c.ws = nullptr; c.ws_bytes = 1; }); }},
    {"conv2d_vjp", "h 0", "bad sizes", [] { return vjp([](Vjp& c) { c.h = 0; }); }},
    {"conv2d_vjp", "kernel size 5", "kernel size", [] { return vjp([](Vjp& c) { c.k = 5; }); }},
    {"conv2d_vjp", "stride 2 with a 1x1 kernel", "mode 0", [] { return vjp([](Vjp& c) { c.mode = 1; c.k = 1; }); }},
    {"conv2d_vjp", "mode 3", "mode 0", [] { return vjp([](Vjp& c) { c.mode = 3; }); }},
    {"conv2d_vjp", "du_raw and g0", "du_raw alone", [] { return vjp([](Vjp& c) { c.raw = Y; }); }},
    {"conv2d_vjp", "neither du_raw nor g0", "du_raw alone", [] { return vjp([](Vjp& c) { c.g0 = nullptr; }); }},
    {"conv2d_vjp", "g1 without c1", "du_raw alone", [] { return vjp([](Vjp& c) { c.g1 = G1; }); }},
    {"conv2d_vjp", "c0 + c1 below cin", "must cover", [] { return vjp([](Vjp& c) { c.c0 = 32; }); }},
    {"conv2d_vjp", "c0 of 68 bf16 channels", "16-byte", [] { return vjp([](Vjp& c) { c.c0 = 68; }); }},
    {"conv2d_vjp", "g_channels 96 for 64", "g_channels", [] { return vjp([](Vjp& c) { c.gch = 96; }); }},
    {"conv2d_vjp", "g_channels 64 for 48 fp32", "g_channels", [] { return vjp([](Vjp& c) { c.dtype = F32; c.cout = 48; c.gch = 64; }); }},
    {"conv2d_vjp", "short workspace", "workspace too small", [] { return vjp([](Vjp& c) { c.ws_bytes = SHORT; }); }},
    {"conv2d_vjp", "short workspace, stride 2, raw", "workspace too small", [] { return vjp([](Vjp& c) { c.mode = 1; c.g0 = nullptr; c.raw = Y; c.ws_bytes = SHORT; }); }},
    // ---- mi355_conv2d_fwd (first HIP call: zeroing the error word, after the workspace check and the route) ----
    {"conv2d_fwd", "null x", "null argument", [] { return fwd([](Fwd& c) { c.x = nullptr; }); }},
    {"conv2d_fwd", "null workspace of 1 byte", "null argument", [] { return fwd([](Fwd& c) { c.ws = nullptr; c.ws_bytes = 1; }); }},
    {"conv2d_fwd", "dtype 7", "dtype", [] { return fwd([](Fwd& c) { c.dtype = BAD; }); }},
    {"conv2d_fwd", "batch 0", "bad sizes", [] { return fwd([](Fwd& c) { c.batch = 0; }); }},
    {"conv2d_fwd", "kernel size 5", "kernel size", [] { return fwd([](Fwd& c) { c.k = 5; }); }},
    {"conv2d_fwd", "stride 3", "stride must be", [] { return fwd([](Fwd& c) { c.stride = 3; }); }},
    {"conv2d_fwd", "resample 3", "pooling", [] { return fwd([](Fwd& c) { c.resample = 3; }); }},
    {"conv2d_fwd", "stride 2 with nearest x2", "combined", [] { return fwd([](Fwd& c) { c.stride = 2; c.resample = 2; }); }},
    {"conv2d_fwd", "stride 2 with a 1x1 kernel", "3x3", [] { return fwd([](Fwd& c) { c.stride = 2; c.k = 1; }); }},
    {"conv2d_fwd", "flag 2", "flag", [] { return fwd([](Fwd& c) { c.flags = 2; }); }},
    {"conv2d_fwd", "x1 without cin1", "go together", [] { return fwd([](Fwd& c) { c.x1 = X1; }); }},
    {"conv2d_fwd", "pro_a without pro_b", "go together", [] { return fwd([](Fwd& c) { c.pro_a = P; }); }},
    {"conv2d_fwd", "res_mode 3", "res_mode", [] { return fwd([](Fwd& c) { c.res = P; c.res_mode = 3; }); }},
    {"conv2d_fwd", "two sources, 64 + 24 bf16 channels", "two-source", [] { return fwd([](Fwd& c) { c.x1 = X1; c.cin1 = 24; }); }},
    {"conv2d_fwd", "NCHW source of 6 + 3 channels", "at most 8", [] { return fwd([](Fwd& c) { c.cin = 6; c.x1 = X1; c.cin1 = 3; c.flags = MI355_CONV_FWD_NCHW_SRC; }); }},
    {"conv2d_fwd", "NCHW source with a prologue", "at most 8", [] { return fwd([](Fwd& c) { c.cin = 3; c.flags = MI355_CONV_FWD_NCHW_SRC; c.pro_a = P; c.pro_b = Q; }); }},
    {"conv2d_fwd", "prologue over 48 bf16 channels", "prologue", [] { return fwd([](Fwd& c) { c.cin = 48; c.pro_a = P; c.pro_b = Q; }); }},
    {"conv2d_fwd", "emb with 3 output channels", "NHWC", [] { return fwd([](Fwd& c) { c.cout = 3; c.emb = P; }); }},
    {"conv2d_fwd", "Euler update with 64 output channels", "Euler", [] { return fwd([](Fwd& c) { c.axpy = G0; }); }},
    {"conv2d_fwd", "short workspace", "workspace too small", [] { return fwd([](Fwd& c) { c.ws_bytes = SHORT; }); }},
    {"conv2d_fwd", "short workspace, phase-eligible nearest x2", "workspace too small", [] { return fwd([](Fwd& c) { c.resample = 2; c.cout = 256; c.h = c.wd = 16; c.ws_bytes = SHORT; }); }},
    // ---- the embedding path and the layout ops (first HIP call: the launch, or the pinned error word) ----
    {"linear", "k 0", "bad argument", [] { return mi355_linear(X, Wt, Bs, Y, 2, 0, 64, 0, 0, nullptr, nullptr); }},
    {"linear", "null out", "bad argument", [] { return mi355_linear(X, Wt, Bs, nullptr, 2, 64, 64, 0, 0, nullptr, nullptr); }},
    {"label_emb_linear", "null err_word", "bad argument", [] { return mi355_label_emb_linear(X, 1, P, LAB, 10, Wt, Bs, Y, 2, 64, 64, nullptr, nullptr, nullptr); }},
    {"label_emb_linear", "null lemb", "bad argument", [] { int32_t e; return mi355_label_emb_linear(X, 1, nullptr, LAB, 10, Wt, Bs, Y, 2, 64, 64, &e, nullptr, nullptr); }},
    {"emb_gather", "j 0", "bad argument", [] { int32_t e; return mi355_emb_gather(X, LAB, 10, Y, 2, 0, &e, nullptr); }},
    {"emb_gather", "null err_word", "bad argument", [] { return mi355_emb_gather(X, LAB, 10, Y, 2, 64, nullptr, nullptr); }},
    {"pack_nhwc", "cond without cc", "bad argument", [] { return mi355_pack_nhwc(X, 3, X1, 0, 2, 64, 8, Y, BF, nullptr); }},
    {"pack_nhwc", "cpad 4 for 3 + 3 channels", "cpad", [] { return mi355_pack_nhwc(X, 3, X1, 3, 2, 64, 4, Y, BF, nullptr); }},
    {"pack_nhwc", "dtype 7", "dtype", [] { return mi355_pack_nhwc(X, 3, nullptr, 0, 2, 64, 8, Y, BAD, nullptr); }},
    {"unpack_nchw", "hw 0", "bad argument", [] { return mi355_unpack_nchw(X, 2, 0, 64, Y, BF, nullptr); }},
    {"unpack_nchw", "dtype 7", "dtype", [] { return mi355_unpack_nchw(X, 2, 64, 64, Y, BAD, nullptr); }},
    {"unpack_channels", "count 0", "bad argument", [] { return mi355_unpack_channels(X, 2, 64, 64, 0, 0, Y, BF, nullptr); }},
    {"unpack_channels", "channels 48 .. 80 of 64", "inside a row", [] { return mi355_unpack_channels(X, 2, 64, 64, 48, 32, Y, BF, nullptr); }},
    {"unpack_channels", "dtype -1", "dtype", [] { return mi355_unpack_channels(X, 2, 64, 64, 0, 32, Y, -1, nullptr); }},
    {"resample", "null out", "bad argument", [] { return mi355_resample(X, nullptr, 2, 8, 8, 64, 2, BF, nullptr); }},
    {"resample", "mode 1", "mode must be", [] { return mi355_resample(X, Y, 2, 8, 8, 64, 1, BF, nullptr); }},
    {"resample", "pool of a 1-row image", "mode must be", [] { return mi355_resample(X, Y, 2, 1, 8, 64, 3, BF, nullptr); }},
    {"resample", "dtype 7", "dtype", [] { return mi355_resample(X, Y, 2, 8, 8, 64, 2, BAD, nullptr); }},
};

bool says(const char* alternatives) {
  const std::string text = mi355_last_error(), alts = alternatives;
  for (size_t i = 0; i <= alts.size();) {
    const size_t j = alts.find('|', i) == std::string::npos ? alts.size() : alts.find('|', i);
    if (text.find(alts.substr(i, j - i)) != std::string::npos) return true;
    i = j + 1;
  }
  return false;
}

// ---- the route queries: what conv_route decides, all words.  Rows: one shape per kernel family tests/conv_fwd_ref.py names (with that table's switches),
// stride 2 and nearest x2, 1x1 and 3x3; each row in every element type the op takes ----
enum { OFF = -1 };   // a switch left at its default
struct RouteRow {
  const char* name; int batch, cin, cin1, cout, h, w, k, stride, up; bool pro, emb; int res_mode; bool nchw, axpy;
  int conv_pp, conv_ws, conv_small, conv_edge, conv_min_wgs;
};
const RouteRow fwd_rows[] = {
    {"igemm 64->128 16x16", 2, 64, 0, 128, 16, 16, 3, 1, 0, false, false, 0, false, false, 0, 0, 0, 0, 1},
    {"igemm s2 64->64 16x16", 2, 64, 0, 64, 16, 16, 3, 2, 0, false, false, 0, false, false, 0, 0, 0, 0, 512},
    {"igemm up 64->64 8x8 silu emb", 2, 64, 0, 64, 8, 8, 3, 1, 1, true, true, 0, false, false, 0, 0, 0, 0, 512},
    {"igemm 1x1 64+32->64 8x8 emb res", 3, 64, 32, 64, 8, 8, 1, 1, 0, false, true, 1, false, false, 0, 0, 0, 0, 512},
    {"1x1 qkv 128->384 8x8", 2, 128, 0, 384, 8, 8, 1, 1, 0, false, false, 0, false, false, 0, OFF, OFF, OFF, OFF},
    {"pp1 256->256 16x16", 1, 256, 0, 256, 16, 16, 1, 1, 0, false, false, 0, false, false, 2, OFF, OFF, OFF, OFF},
    {"pp1 512x128 256->128 32x16", 1, 256, 0, 128, 32, 16, 1, 1, 0, false, false, 0, false, false, 2, OFF, OFF, OFF, OFF},
    {"pp1 128x256 256->256 16x16", 2, 256, 0, 256, 16, 16, 1, 1, 0, false, false, 0, false, false, 34, OFF, OFF, OFF, OFF},
    {"in 3->128 16x16", 2, 3, 0, 128, 16, 16, 3, 1, 0, false, false, 0, false, false, OFF, OFF, OFF, OFF, OFF},
    {"in nchw 3+3->128 48x16", 2, 3, 3, 128, 48, 16, 3, 1, 0, false, false, 0, true, false, OFF, OFF, OFF, OFF, OFF},
    {"in nchw off 3+3->128 16x16", 2, 3, 3, 128, 16, 16, 3, 1, 0, false, false, 0, true, false, OFF, OFF, OFF, 11, OFF},
    {"out 128->3 16x16 silu", 2, 128, 0, 3, 16, 16, 3, 1, 0, true, false, 0, false, false, OFF, OFF, OFF, OFF, OFF},
    {"out 128->3 16x16 silu axpy", 2, 128, 0, 3, 16, 16, 3, 1, 0, true, false, 0, false, true, OFF, OFF, OFF, OFF, OFF},
    {"out 256->3 20x28 silu", 1, 256, 0, 3, 20, 28, 3, 1, 0, true, false, 0, false, false, OFF, OFF, OFF, OFF, OFF},
    {"pp wide 64->256 16x16", 1, 64, 0, 256, 16, 16, 3, 1, 0, false, false, 0, false, false, 94, 0, 0, OFF, OFF},
    {"pp wide silu 128->256 16x16 res up2", 2, 128, 0, 256, 16, 16, 3, 1, 0, true, false, 2, false, false, 94, 0, 0, OFF, OFF},
    {"pp narrow 64->128 16x32", 1, 64, 0, 128, 16, 32, 3, 1, 0, false, false, 0, false, false, 94, 0, 0, OFF, OFF},
    {"pp phase 64->256 16x16", 1, 64, 0, 256, 16, 16, 3, 1, 1, false, false, 0, false, false, 94, 0, 0, OFF, OFF},
    {"pp up, phase form off, 128->256 8x8", 2, 128, 0, 256, 8, 8, 3, 1, 1, false, false, 0, false, false, 30, 0, 0, OFF, OFF},
    {"ws 64->128 16x16", 1, 64, 0, 128, 16, 16, 3, 1, 0, false, false, 0, false, false, 0, 5, 0, OFF, 1},
    {"ws cat 32+96->128 20x20 silu", 1, 32, 96, 128, 20, 20, 3, 1, 0, true, false, 0, false, false, 0, 5, 0, OFF, 1},
    {"ws up 64->128 8x8", 2, 64, 0, 128, 8, 8, 3, 1, 1, false, false, 0, false, false, 0, 5, 0, OFF, 1},
    {"small 8x8 128->128 B2", 2, 128, 0, 128, 8, 8, 3, 1, 0, false, false, 0, false, false, 0, 0, 15, OFF, OFF},
    {"small 8x8 32->256 B256", 256, 32, 0, 256, 8, 8, 3, 1, 0, false, false, 0, false, false, 0, 0, 15, OFF, OFF},
    {"small s2 128->128 16->8", 2, 128, 0, 128, 16, 16, 3, 2, 0, false, false, 0, false, false, 0, 0, 15, OFF, OFF},
    {"small up 128->128 4->8 emb", 2, 128, 0, 128, 4, 4, 3, 1, 1, false, true, 0, false, false, 0, 0, 15, OFF, OFF},
    {"defaults 128->128 32x32 B64", 64, 128, 0, 128, 32, 32, 3, 1, 0, false, false, 0, false, false, OFF, OFF, OFF, OFF, OFF},
    {"defaults up 256->256 16x16 B64", 64, 256, 0, 256, 16, 16, 3, 1, 1, false, false, 0, false, false, OFF, OFF, OFF, OFF, OFF},
};
// the data-gradient conv: name, batch, cout, cin, c0, c1, h, w, k, mode (0 unit, 1 stride 2, 2 nearest x2), switches
struct VjpRow { const char* name; int batch, cout, cin, c0, c1, h, w, k, mode, conv_pp, conv_ws, conv_small, conv_min_wgs; };
const VjpRow vjp_rows[] = {
    {"3x3 128->128 16x16", 2, 128, 128, 128, 0, 16, 16, 3, 0, OFF, OFF, OFF, OFF},
    {"3x3 128->128 16x16 plain tiles", 2, 128, 128, 128, 0, 16, 16, 3, 0, 0, 0, 0, 512},
    {"3x3 cat 64+64->128 16x16", 2, 128, 128, 64, 64, 16, 16, 3, 0, OFF, OFF, OFF, OFF},
    {"3x3 3->128 16x16 (first conv)", 2, 128, 3, 8, 0, 16, 16, 3, 0, OFF, OFF, OFF, OFF},
    {"3x3 128->3 16x16 (out conv)", 2, 3, 128, 128, 0, 16, 16, 3, 0, OFF, OFF, OFF, OFF},
    {"1x1 256->128 8x8", 2, 128, 256, 256, 0, 8, 8, 1, 0, OFF, OFF, OFF, OFF},
    {"1x1 128->384 16x16", 2, 384, 128, 128, 0, 16, 16, 1, 0, OFF, OFF, OFF, OFF},
    {"s2 128->128 16x16", 2, 128, 128, 128, 0, 16, 16, 3, 1, OFF, OFF, OFF, OFF},
    {"s2 128->128 15x15", 2, 128, 128, 128, 0, 15, 15, 3, 1, OFF, OFF, OFF, OFF},
    {"up 128->128 8x8", 2, 128, 128, 128, 0, 8, 8, 3, 2, OFF, OFF, OFF, OFF},
    {"up 256->256 16x16 B64", 64, 256, 256, 256, 0, 16, 16, 3, 2, OFF, OFF, OFF, OFF},
    {"small 8x8 128->128", 2, 128, 128, 128, 0, 8, 8, 3, 0, 0, 0, 15, OFF},
    {"small 4x4 256->128 B5", 5, 128, 256, 256, 0, 4, 4, 3, 0, 0, 0, 15, OFF},
    {"ws 128->128 32x32 B64", 64, 128, 128, 128, 0, 32, 32, 3, 0, 0, 5, 0, 1},
    {"pp 256->256 16x16 B64", 64, 256, 256, 256, 0, 16, 16, 3, 0, 94, 0, 0, OFF},
};
mi355_debug_config switches(int pp, int ws, int small, int edge, int min_wgs) {
  mi355_debug_config k = knobs();
  if (pp != OFF) k.conv_pp = pp;
  if (ws != OFF) k.conv_ws = ws;
  if (small != OFF) k.conv_small = small;
  if (edge != OFF) k.conv_edge = edge;
  if (min_wgs != OFF) k.conv_min_wgs = min_wgs;
  return k;
}
void print_route(const char* op, const char* row, const char* type, int rc, const int32_t* r, int n) {
  printf("  %s | %s | %s | %d |", op, row, type, rc);
  for (int i = 0; i < n; ++i) printf(" %d", r[i]);
  printf("%s%s\n", rc ? " | " : "", rc ? mi355_last_error() : "");
}
// a route query never reaches HIP: -3 fails the program; a shape a type has no route for is an answer like any other
int route_tables() {
  int bad = 0;
  const struct { int code; const char* name; } types[4] = {{F32, "fp32"}, {BF, "bf16"}, {X2, "bf16x2"}, {F16, "fp16"}};
  printf("conv2d_fwd route query: kernel form tile_m tile_n reads_nchw axpy ksplit n_mt\n");
  for (const RouteRow& q : fwd_rows)
    for (const auto& t : types) {
      const mi355_debug_config k = switches(q.conv_pp, q.conv_ws, q.conv_small, q.conv_edge, q.conv_min_wgs);
      int32_t r[8];
      Fwd c; c.x = nullptr; c.w = nullptr; c.y = nullptr; c.ws = nullptr; c.ws_bytes = 0; c.route = r; c.debug = &k; c.dtype = t.code;
      c.batch = q.batch; c.cin = q.cin; c.cin1 = q.cin1; c.cout = q.cout; c.h = q.h; c.wd = q.w; c.k = q.k; c.stride = q.stride; c.resample = q.up ? 2 : 0;
      if (q.pro) { c.pro_a = P; c.pro_b = Q; c.pro_silu = 1; }
      if (q.emb) c.emb = P;
      if (q.res_mode) { c.res = Q; c.res_mode = q.res_mode; }
      if (q.nchw) c.flags = MI355_CONV_FWD_NCHW_SRC;
      if (q.axpy) c.axpy = G0;
      const int rc = c.call();
      print_route("conv2d_fwd", q.name, t.name, rc, r, 8);
      bad += rc == MI355_ERR_HIP;
    }
  printf("conv2d_vjp route query: kernel form tile_m tile_n\n");
  for (const VjpRow& q : vjp_rows)
    for (const auto& t : types) {
      if (t.code != F32 && t.code != BF) continue;
      const mi355_debug_config k = switches(q.conv_pp, q.conv_ws, q.conv_small, OFF, q.conv_min_wgs);
      const int ch = t.code == F32 ? 16 : 32;
      int32_t r[4];
      Vjp c; c.w = nullptr; c.go = nullptr; c.g0 = nullptr; c.ws = nullptr; c.ws_bytes = 0; c.route = r; c.debug = &k; c.dtype = t.code;
      c.batch = q.batch; c.cout = q.cout; c.cin = q.cin; c.c0 = q.c0; c.c1 = q.c1; c.h = q.h; c.wd = q.w; c.k = q.k; c.mode = q.mode; c.gch = (q.cout + ch - 1) / ch * ch;
      const int rc = c.call();
      print_route("conv2d_vjp", q.name, t.name, rc, r, 4);
      bad += rc == MI355_ERR_HIP;
    }
  return bad;
}

}  // namespace

int main() {
  // Every faulted call below is meant to be refused on the host; one that is not would reach HIP with made-up addresses.  Where a GPU driver is
  // present that is a memory fault on a device others may share, so the program does not run there at all.
  if (access("/dev/kfd", F_OK) == 0) {
    fprintf(stderr, "op_refusals: this machine has a GPU driver node (/dev/kfd); the program runs on machines without a device only\n");
    return 2;
  }
  int bad = 0;
  printf("refusals: op | fault | return code | message\n");
  for (const Case& c : cases) {
    const int rc = c.call();
    printf("  %s | %s | %d | %s\n", c.op, c.what, rc, rc ? mi355_last_error() : "");
    if (rc != 0 && rc != MI355_ERR_HIP && says(c.expect)) continue;
    printf("  ^ FAILED: %s\n", rc == 0 || rc == MI355_ERR_HIP ? "not refused on the host" : "refused for another reason than the fault made");
    ++bad;
  }
  bad += route_tables();
  if (bad) fprintf(stderr, "%d cases failed\n", bad);
  return bad ? 1 : 0;
}
