// Host-side weight packers of the implicit-GEMM conv families (no kernel): the packed images conv_igemm.hip, conv_ws.hip, conv_pp.hip, conv_pp1.hip,
// conv_small.hip, conv1x1.hip and attn_fused.hip read, and their sizes.
#include <cstring>
#include <vector>

#include "ops.h"

int conv_tile_n(int Cout) {
  if (Cout % 128 == 0) return 128;
  if (Cout % 64 == 0) return 64;
  return 32;
}

static inline int chunk_of(int dtype) { return dtype == 0 ? 16 : 32; }

size_t conv_packed_weight_bytes(int dtype, int Cout, int Cin, int ks, int split) {
  const int BN = conv_tile_n(Cout), CH = chunk_of(dtype);
  const size_t nt = (Cout + BN - 1) / BN, nc = (size_t)((Cin + CH - 1) / CH) * (split ? 2 : 1);
  return nt * nc * ks * ks * (size_t)BN * 64;
}

static inline uint16_t f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
static inline float bf2f(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

// A packed weight image is a sequence of [BN rows][64 B] tiles, one per (output-channel tile, K chunk, tap): a row holds one chunk of CH input
// channels as four 16-byte quads of V elements, quad q at slot q ^ ((row >> 1) & 3) (the swizzle the kernels' LDS reads undo, brow above).
namespace {
struct PackTile {
  int dtype, BN, CH, V, esz;
  PackTile(int dtype_, int Cout) : dtype(dtype_), BN(conv_tile_n(Cout)), CH(chunk_of(dtype_)), V(CH / 4), esz(dtype_ == 0 ? 4 : 2) {}
  // element kl of the chunk, output channel `row` of the tile: v rounded to the image's element type
  void store(char* tile, int row, int kl, float v) const {
    const int q = kl / V, e = kl % V;
    char* dstp = tile + row * 64 + 16 * (q ^ ((row >> 1) & 3)) + e * esz;
    if (dtype == DT_F32) memcpy(dstp, &v, 4);
    else if (dtype == DT_F16) { const _Float16 h = (_Float16)v; memcpy(dstp, &h, 2); }   // RNE
    else { uint16_t h = f2bf(v); memcpy(dstp, &h, 2); }
  }
};
}  // namespace

void conv_pack_weights(int dtype, const float* w, int Cout, int Cin, int ks, void* dst, int split) {
  const PackTile pk(dtype, Cout);
  const int BN = pk.BN, CH = pk.CH;
  const int nt = (Cout + BN - 1) / BN, nr = (Cin + CH - 1) / CH, nc = nr * (split && dtype == 1 ? 2 : 1), ntaps = ks * ks;
  char* out = reinterpret_cast<char*>(dst);
  memset(out, 0, conv_packed_weight_bytes(dtype, Cout, Cin, ks, split));
  for (int t = 0; t < nt; ++t)
    for (int c = 0; c < nc; ++c)
      for (int tap = 0; tap < ntaps; ++tap) {
        char* tile = out + (((size_t)t * nc + c) * ntaps + tap) * (size_t)BN * 64;
        const bool lo = c >= nr;               // second half of the K loop: the rounding residual of the first half's weights
        for (int row = 0; row < BN; ++row) {
          const int co = t * BN + row;
          if (co >= Cout) break;
          for (int kl = 0; kl < CH; ++kl) {
            const int ci = (lo ? c - nr : c) * CH + kl;
            if (ci >= Cin) break;
            float v = w[((size_t)co * Cin + ci) * ntaps + tap];
            if (lo) v = v - bf2f(f2bf(v));
            pk.store(tile, row, kl, v);
          }
        }
      }
}

// Nearest-x2 up-sample followed by a 3x3 conv (padding 1) = four 2x2 convs of the low-res image, one per output phase (a, b) = (row, column parity):
// output row 2 i + a reads high-res rows 2 i + a - 1 .. 2 i + a + 1 = low-res rows {i - 1, i, i} (a = 0) or {i, i, i + 1} (a = 1), so tap ky' of the
// phase filter is the sum of the 3x3 rows ky with (a + ky + 1) / 2 == a + ky' (and the same along x).  Summed in fp32, then rounded and swizzled per
// element exactly as conv_pack_weights does.  Layout per 128-row pack tile: [phase 2 a + b][chunk][tap 2 ky' + kx'][128 rows][64 B].
size_t conv_packed_weight_bytes_up2(int dtype, int Cout, int Cin) {
  const int BN = conv_tile_n(Cout), CH = chunk_of(dtype);
  const size_t nt = (Cout + BN - 1) / BN, nc = (size_t)((Cin + CH - 1) / CH);
  return nt * 4 * nc * 4 * (size_t)BN * 64;
}
void conv_pack_weights_up2(int dtype, const float* w, int Cout, int Cin, void* dst) {
  const PackTile pk(dtype, Cout);
  const int BN = pk.BN, CH = pk.CH;
  const int nt = (Cout + BN - 1) / BN, nc = (Cin + CH - 1) / CH;
  char* out = reinterpret_cast<char*>(dst);
  memset(out, 0, conv_packed_weight_bytes_up2(dtype, Cout, Cin));
  for (int t = 0; t < nt; ++t)
    for (int ph = 0; ph < 4; ++ph)
      for (int c = 0; c < nc; ++c)
        for (int tap = 0; tap < 4; ++tap) {
          const int pa = ph >> 1, pb = ph & 1, ty = tap >> 1, tx = tap & 1;
          char* tile = out + ((((size_t)t * 4 + ph) * nc + c) * 4 + tap) * (size_t)BN * 64;
          for (int row = 0; row < BN; ++row) {
            const int co = t * BN + row;
            if (co >= Cout) break;
            for (int kl = 0; kl < CH; ++kl) {
              const int ci = c * CH + kl;
              if (ci >= Cin) break;
              const float* w9 = w + ((size_t)co * Cin + ci) * 9;
              float v = 0.f;
              for (int ky = 0; ky < 3; ++ky)
                for (int kx = 0; kx < 3; ++kx)
                  if ((pa + ky + 1) / 2 == pa + ty && (pb + kx + 1) / 2 == pb + tx) v += w9[ky * 3 + kx];
              pk.store(tile, row, kl, v);
            }
          }
        }
}

size_t conv_packed_weight_bytes_skip(int dtype, int Cout, int Cin, int Cskip) {
  return conv_packed_weight_bytes(dtype, Cout, Cin, 3, 0) + conv_packed_weight_bytes(dtype, Cout, Cskip, 1, 0);
}
void conv_pack_weights_skip(int dtype, const float* w3, const float* w1, int Cout, int Cin, int Cskip, void* dst) {
  const size_t b3 = conv_packed_weight_bytes(dtype, Cout, Cin, 3, 0), b1 = conv_packed_weight_bytes(dtype, Cout, Cskip, 1, 0);
  std::vector<char> t3(b3), t1(b1);
  conv_pack_weights(dtype, w3, Cout, Cin, 3, t3.data(), 0);
  conv_pack_weights(dtype, w1, Cout, Cskip, 1, t1.data(), 0);
  const size_t nt = (Cout + conv_tile_n(Cout) - 1) / conv_tile_n(Cout), s3 = b3 / nt, s1 = b1 / nt;
  char* out = reinterpret_cast<char*>(dst);
  for (size_t t = 0; t < nt; ++t) {
    memcpy(out + t * (s3 + s1), t3.data() + t * s3, s3);
    memcpy(out + t * (s3 + s1) + s3, t1.data() + t * s1, s1);
  }
}

// Weights of the data-gradient conv (backward w.r.t. the input) of a [Cout][Cin][ks][ks] forward filter: the transposed conv of a
// stride-1, padding ks/2 convolution is the same convolution with input / output channels swapped and the taps flipped,
// W'[ci][co][ky][kx] = W[co][ci][ks-1-ky][ks-1-kx]; rows ci >= Cin (channel padding of the forward input) are zero.
size_t conv_packed_weight_bytes_dgrad(int dtype, int Cout, int Cin, int ks, int cin_pad) { (void)Cin; return conv_packed_weight_bytes(dtype, cin_pad, Cout, ks); }
void conv_pack_weights_dgrad(int dtype, const float* w, int Cout, int Cin, int ks, int cin_pad, void* dst) {
  const int nt = ks * ks;
  std::vector<float> t((size_t)cin_pad * Cout * nt, 0.f);
  for (int co = 0; co < Cout; ++co)
    for (int ci = 0; ci < Cin; ++ci)
      for (int tap = 0; tap < nt; ++tap) t[((size_t)ci * Cout + co) * nt + (nt - 1 - tap)] = w[((size_t)co * Cin + ci) * nt + tap];
  conv_pack_weights(dtype, t.data(), cin_pad, Cout, ks, dst);
}
