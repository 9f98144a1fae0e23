// Device noise: Philox4x32-10 + Box-Muller keyed by (seed, counter).  Counter c yields elements 4c .. 4c + 3 of the stream, so element i of a
// tensor drawn at Philox offset `offset` (a multiple of 4) is lane i & 3 of counter offset / 4 + (i >> 2) whichever kernel asks for it: the step
// kernels that consume a draw (steps.hip) and the kernels that regenerate one instead of storing it (vlb.hip).
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

// the uniform -> normal map is written operation by operation; an includer with contraction on would change the draws
#pragma clang fp contract(off)

namespace {

struct Philox {
  static constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  __device__ static inline void round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    const uint64_t p0 = (uint64_t)M0 * c[0], p1 = (uint64_t)M1 * c[2];
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c[0] = hi1 ^ c[1] ^ k0; c[1] = lo1; c[2] = hi0 ^ c[3] ^ k1; c[3] = lo0;
  }
  __device__ static inline void gen(uint64_t seed, uint64_t ctr, uint32_t (&out)[4]) {
    uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), 0u, 0u};
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int i = 0; i < 10; ++i) { round(c, k0, k1); k0 += W0; k1 += W1; }
    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
  }
};

// 4 standard normals for counter `ctr` (elements 4*ctr .. 4*ctr+3 of the stream)
__device__ inline void randn4(uint64_t seed, uint64_t ctr, float (&z)[4]) {
  uint32_t r[4];
  Philox::gen(seed, ctr, r);
  const float k = 2.3283064365386963e-10f;  // 2^-32
  const float u0 = ((float)r[0] + 0.5f) * k, u1 = ((float)r[1] + 0.5f) * k;
  const float u2 = ((float)r[2] + 0.5f) * k, u3 = ((float)r[3] + 0.5f) * k;
  const float ra = sqrtf(-2.0f * logf(fminf(fmaxf(u0, 1e-12f), 1.0f))), rb = sqrtf(-2.0f * logf(fminf(fmaxf(u2, 1e-12f), 1.0f)));
  const float ta = 6.283185307179586f * u1, tb = 6.283185307179586f * u3;
  z[0] = ra * cosf(ta); z[1] = ra * sinf(ta); z[2] = rb * cosf(tb); z[3] = rb * sinf(tb);
}

}  // namespace
