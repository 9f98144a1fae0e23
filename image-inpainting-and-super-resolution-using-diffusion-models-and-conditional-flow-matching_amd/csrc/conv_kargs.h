// What the 3x3 / 1x1 implicit-GEMM conv families share (conv_igemm.hip, conv_ws.hip, conv_pp.hip, conv_pp1.hip, conv_small.hip): the kernels' argument
// block, the device helpers every family uses, the diagnostic stamp macros, and what conv_route hands a family's *_route / *_launch (ops.h).
// ConvKArgs and the helpers stay in an unnamed namespace: the kernels' mangled names (_ZN12_GLOBAL__N_1...), which the profiles and tools key on,
// contain it.  Every unit therefore has its own copy of these types, identical because they all come from this header.
#pragma once
#include "ops.h"

#ifndef WS_ABLATE
#define WS_ABLATE 0   // diagnostic builds only (make variant ABL=<mask>): the warp-specialised and the small-level kernel read it (conv_ws.inc.h, conv_small.inc.h)
#endif

namespace {

constexpr int PROW = 96;   // bytes per patch pixel row in LDS (64 data + 32 pad)

struct ConvKArgs {
  const void* src0; const void* src1;
  int C0, C1, Cin, nchunks;          // nchunks: 64-byte K chunks of the packed weights (2 x nreal with hi / lo split weights, else nreal)
  int nreal;                         // 64-byte channel chunks of the activations: weight chunk c contracts with activation chunk c mod nreal
  int N, Hs, Ws, Hc, Wc, Ho, Wo;
  int mode, pad, stride;
  const float* pro_a; const float* pro_b; int pro_silu;
  const void* w; const float* bias; int Cout; int bn_pack;
  const float* emb; int emb_stride;
  const void* res; int res_mode; int Hr, Wr;
  void* out; int out_mode;
  float* gn_stats; int gn_slots;     // fused GroupNorm partial sums of the output (common.h GnPartial), or null
  int lvw, lth, G, PW, PH, NP, tiles_x, tiles_y;
  uint32_t bytes0, bytes1, wbytes, obytes, rbytes;   // buffer sizes (raw buffer descriptors: out-of-range loads return 0, stores drop)
  unsigned long long* dbg;           // diagnostic build only (-DCONV_STAMPS): per-phase cycle sums
  int ablate;                        // diagnostic build only: 1 = no output stores, 2 = no prologue math, 4 = no MFMA
  int stagger;                       // odd-slot workgroup start delay in units of s_sleep(127) (~8k cycles each)
  uint32_t* err;                     // error word (device-visible): bit 0 = a counter wait of the persistent kernel expired
  int spin_limit;                    // polls before such a wait gives up
  // small-level kernel only (conv_small.inc.h): the GroupNorm site that reads this conv's output is applied in the epilogue - a wave
  // holds whole images x 64 channels = whole groups, so act_out = silu?(GN(out)) needs no pass of its own; out itself is written
  // only if somebody else reads it (act_raw); one touch of the NEXT conv's packed weights (the pass's L2 warm-up moves here too)
  void* act_out; const float* act_gamma; const float* act_beta; const float* act_film; int act_film_stride; float act_eps;
  int act_silu, act_raw;
  int act_stride, act_coff, act_cpg; uint32_t abytes;   // act_out: channels per pixel, first channel this conv fills, channels per group, bytes
  void* act2_out; const float* act2_gamma; const float* act2_beta; int act2_silu, act2_stride, act2_coff, act2_cpg; uint32_t a2bytes;   // a second site (no FiLM)
  const void* warm; uint32_t warm_bytes;
  // small-level kernel only: a 1x1 conv of cat(sk0, sk1) (SC0 + SC1 channels at the output resolution) accumulated into the same output - the
  // ResBlock's skip_connection inside its second conv; w then holds, per 128-channel pack tile, the 3x3 tiles followed by one tile per skip chunk
  const void* sk0; const void* sk1; int SC0, SC1; uint32_t skbytes0, skbytes1;
  uint32_t wstride;                  // 8-KB weight tiles per 128-channel pack tile (9 nchunks without a fused skip conv)
};

#ifdef CONV_STAMPS
// In-kernel phase stamps (cdna_hip_programming.md section 7): diagnostic build only, never the timed build.
__device__ __forceinline__ unsigned long long conv_stamp() {
  unsigned long long t;
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  __builtin_amdgcn_sched_barrier(0);
  return t;
}
#define STAMP_DECL unsigned long long st_prev = conv_stamp(), st_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define STAMP(k) { const unsigned long long st_now = conv_stamp(); st_acc[k] += st_now - st_prev; st_prev = st_now; }
#define STAMP_FLUSH if (p.dbg && (threadIdx.x & 63) == 0) { unsigned long long* q = p.dbg + ((size_t)(blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x / 64) + (threadIdx.x >> 6)) * 8; for (int k = 0; k < 8; ++k) q[k] = st_acc[k]; }
// In-kernel clock of a wave (MI355X_MICROARCH.md, DVFS give-back item 6): shader-clock cycles per 100-MHz reference tick over the wave's
// life time; two u64 per wave in the 64 KB in FRONT of the stamp buffer (the persistent conv's consumer waves only).
#define CLK_DECL const unsigned long long ck_t0 = __builtin_amdgcn_s_memtime(), ck_r0 = __builtin_amdgcn_s_memrealtime();
#define CLK_FLUSH if (p.dbg && (threadIdx.x & 63) == 0) { unsigned long long* q = p.dbg - 8192 + ((size_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6)) * 2; q[0] = __builtin_amdgcn_s_memtime() - ck_t0; q[1] = __builtin_amdgcn_s_memrealtime() - ck_r0; }
#else
#define STAMP_DECL
#define STAMP(k)
#define STAMP_FLUSH
#define CLK_DECL
#define CLK_FLUSH
#endif

template <int I> struct IC { static constexpr int value = I; };

// activation chunk of weight chunk c (hi / lo split weights: the second half of the K loop runs over the same activations again)
__device__ __forceinline__ int src_chunk(const ConvKArgs& p, int c) { return c >= p.nreal ? c - p.nreal : c; }

template <bool FAST> __device__ __forceinline__ float silu_fast(float v) {
  if (FAST) return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * v));
  return v / (1.0f + expf(-v));
}

__device__ __forceinline__ u32x4 buf_load16(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}

}  // namespace

// The plain kernel's tiling of a description (conv_igemm.hip compute_geo)
struct Geo {
  int Hc, Wc, Ho, Wo, BM, BN, bn_pack, lvw, lth, G, PW, PH, NP, tiles_x, tiles_y, groups, pad, stride, plane_bytes, pit, pit_t;
  size_t lds;
};

// What conv_route / conv_launch have worked out for a description when they ask ws / pp / small (ops.h): the plain tiling, the plain kernel's
// arguments (every family's launch starts from them), the knobs in force and the three facts more than one family asks for.
struct ConvPre {
  Geo g;
  ConvKArgs a;
  const mi355_debug_config* K;
  bool gn_ok;      // the description wants output GroupNorm statistics and its shape lets a conv epilogue produce them
  bool has_pro;    // GroupNorm affine (+ SiLU) prologue
  bool fskip;      // a fused 1x1 skip conv (ConvDesc::skip_src0)
};

int ws_num_cus();   // CUs of the current device (256 where there is none): the persistent kernels' grid and the "every CU gets a tile" rules
// grid of a persistent kernel that walks n_mt pixel tiles x n_nt channel tiles (the host half of TileWalk, conv_epilogue.h): one workgroup per CU,
// fewer where the walk has fewer items
inline int persistent_grid(int n_mt, int n_nt) {
  const int ntp = ((n_mt + 7) / 8) * 8 * n_nt, ncu = ws_num_cus();
  return ntp < ncu ? ntp : ncu;
}
