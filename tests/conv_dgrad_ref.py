"""The data gradient of one convolution of the U-Net, three ways, and the case table of its tests.

  dgrad_autograd     the reference: torch.autograd.grad through F.conv2d(cat(x0, x1), W, stride, padding = k // 2), or through
                     F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), W, padding=1) for the nearest-x2 form, in any dtype
  dgrad_decomposed   what csrc/unet_backward.hip conv_dgrad_launch does, in plain torch: the transposed, tap-flipped filter
                     W'[ci][co][ky][kx] = W[co][ci][k-1-ky][k-1-kx] (conv_pack_weights_dgrad), zero insertion for stride 2, one stride-1 conv,
                     2x2 block sums for nearest x2, zero channels up to cin_pad, the split at c0
  CASES              the shapes tests/test_gpu_conv_dgrad.py runs; tests/test_conv_dgrad_ref_cpu.py holds the decomposition to autograd on small
                     shapes and runs conv_route over this table on the CPU (every kernel a bias-free NHWC unit-mode conv can take is reached)

Modes: 0 plain, 1 stride 2, 2 nearest x2 before the conv (csrc/ops.h ConvMode).  The conv is linear: the point the gradient is taken at is zero.
"""
import torch
import torch.nn.functional as F

UNIT, STRIDE2, UP2 = 0, 1, 2


def out_size(h, w, mode):
    """Spatial size of the forward conv's output for an h x w input (k = 3 and padding 1 for the resampling modes)."""
    if mode == STRIDE2:
        return (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if mode == UP2:
        return 2 * h, 2 * w
    return h, w


def cin_pad_of(c0, c1):
    return (c0 + c1 + 31) // 32 * 32


def dgrad_autograd(W, G, c0, c1, h, w, mode, dtype=torch.float64, with_hi=False):
    """-> (grad of x0 [B, c0, h, w], grad of x1 [B, c1, h, w] or None) for the cotangent G of conv(cat(x0, x1)[:, :Ci]); W [Co, Ci, k, k] with
    Ci <= c0 + c1 (the channels beyond Ci are padding the conv never reads).  with_hi (nearest x2): also the gradient of the up-sampled tensor
    [B, Ci, 2h, 2w], whose 2x2 block sums the other two are."""
    Co, Ci, k, _ = W.shape
    B = G.shape[0]
    leaves = [torch.zeros(B, c0, h, w, dtype=dtype, requires_grad=True)]
    if c1:
        leaves.append(torch.zeros(B, c1, h, w, dtype=dtype, requires_grad=True))
    x = torch.cat(leaves, dim=1)[:, :Ci]
    hi = F.interpolate(x, scale_factor=2, mode="nearest") if mode == UP2 else x
    y = F.conv2d(hi, W.to(dtype), stride=2 if mode == STRIDE2 else 1, padding=k // 2)
    assert y.shape == G.shape, (y.shape, G.shape)
    want = leaves + ([hi] if with_hi and mode == UP2 else [])
    g = torch.autograd.grad((y * G.to(dtype)).sum(), want)
    out = (g[0], g[1] if c1 else None)
    return out + ((g[-1] if mode == UP2 else None),) if with_hi else out


def dgrad_decomposed(W, G, c0, c1, h, w, mode, dtype=torch.float64):
    """The engine's sequence.  -> (g0, g1 or None, raw [B, cin_pad, h, w]): raw is the buffer the GroupNorm adjoint reads."""
    Co, Ci, k, _ = W.shape
    B = G.shape[0]
    Ho, Wo = out_size(h, w, mode)
    assert tuple(G.shape) == (B, Co, Ho, Wo)
    Wt = W.to(dtype).flip(2, 3).transpose(0, 1).contiguous()          # [Ci, Co, k, k]
    Gd = G.to(dtype)
    if mode == STRIDE2:                                              # zero insertion: Z[2 y, 2 x] = G[y, x] at the input resolution
        Z = torch.zeros(B, Co, h, w, dtype=dtype)
        Z[:, :, 0:2 * Ho:2, 0:2 * Wo:2] = Gd
        Gd = Z
    D = F.conv2d(Gd, Wt, padding=k // 2)                              # [B, Ci, h, w], or at 2h x 2w for nearest x2
    if mode == UP2:
        D = D.reshape(B, Ci, h, 2, w, 2).sum(dim=(3, 5))
    raw = torch.zeros(B, cin_pad_of(c0, c1), h, w, dtype=dtype)
    raw[:, :Ci] = D
    return raw[:, :c0], (raw[:, c0:c0 + c1] if c1 else None), raw


# ---- the GPU test's table --------------------------------------------------------------------------------------------------------------
# name, B, Co, Ci, c0, c1, h, w (of the forward input), k, mode, forms.  c0 = None: one chunk of the element type (16 fp32 / 32 bf16 channels: the
# network input padded, Ci of them real).  forms: "raw", or (acc0, acc1) for the scatter into (g0, g1).
FF = (False, False)
ACCS = [(False, False), (True, False), (False, True), (True, True)]
CASES = [
    # the out conv's adjoint: G padded to one chunk, 3 of its channels real
    ("out 128->3 16x16", 2, 3, 128, 128, 0, 16, 16, 3, UNIT, ["raw"]),
    ("out 128->3 20x28", 1, 3, 128, 128, 0, 20, 28, 3, UNIT, ["raw"]),
    # the first conv's adjoint: 1, 3, 6 real input channels of a chunk, cin_pad 32
    ("first 1->128", 2, 128, 1, None, 0, 16, 16, 3, UNIT, ["raw", FF]),
    ("first 3->128", 2, 128, 3, None, 0, 16, 16, 3, UNIT, ["raw", FF]),
    ("first 6->128", 2, 128, 6, None, 0, 16, 16, 3, UNIT, ["raw", (True, False)]),
    # plain 3x3
    ("3x3 32->32 4x4", 9, 32, 32, 32, 0, 4, 4, 3, UNIT, ["raw", FF]),
    ("3x3 64->64 7x7", 3, 64, 64, 64, 0, 7, 7, 3, UNIT, ["raw", (True, False)]),
    ("3x3 96->32 8x8", 2, 32, 96, 96, 0, 8, 8, 3, UNIT, ["raw"]),
    ("3x3 32->96 8x8", 2, 96, 32, 32, 0, 8, 8, 3, UNIT, ["raw"]),
    ("3x3 64->128 14x14", 2, 128, 64, 64, 0, 14, 14, 3, UNIT, ["raw"]),
    ("3x3 128->128 16x16", 2, 128, 128, 128, 0, 16, 16, 3, UNIT, ["raw", FF]),
    ("3x3 128->128 32x32", 2, 128, 128, 128, 0, 32, 32, 3, UNIT, ["raw"]),
    # 1x1: qkv (128 -> 384), proj / skip
    ("1x1 qkv 8x8", 2, 384, 128, 128, 0, 8, 8, 1, UNIT, ["raw"]),
    ("1x1 qkv 16x16", 2, 384, 128, 128, 0, 16, 16, 1, UNIT, ["raw"]),
    ("1x1 256->128 8x8", 2, 128, 256, 256, 0, 8, 8, 1, UNIT, ["raw", (True, False)]),
    ("1x1 96->64 8x8", 2, 64, 96, 96, 0, 8, 8, 1, UNIT, [FF]),
    # stride 2 (Downsample: no prologue, the scatter form)
    ("s2 64->64 16x16", 2, 64, 64, 64, 0, 16, 16, 3, STRIDE2, [FF]),
    ("s2 32->32 7x7", 2, 32, 32, 32, 0, 7, 7, 3, STRIDE2, [FF, (True, False)]),
    ("s2 32->64 8x6", 2, 64, 32, 32, 0, 8, 6, 3, STRIDE2, [FF]),
    # nearest x2: Upsample.conv (scatter) and ResBlock(up) (prologue: raw, block sums through tmp)
    ("up 64->64 8x8", 2, 64, 64, 64, 0, 8, 8, 3, UP2, ["raw", FF]),
    ("up 64->64 4x4", 2, 64, 64, 64, 0, 4, 4, 3, UP2, ["raw", (True, False)]),
    ("up 128->64 8x8", 2, 64, 128, 128, 0, 8, 8, 3, UP2, ["raw", FF]),
    ("up 128->64 4x4", 2, 64, 128, 128, 0, 4, 4, 3, UP2, ["raw", FF]),
    # two sources (the skip concat): 3x3 and the 1x1 skip conv over a concat
    ("cat 64+32 3x3", 2, 64, 96, 64, 32, 8, 8, 3, UNIT, ACCS + ["raw"]),
    ("cat 128+128 3x3", 2, 128, 256, 128, 128, 8, 8, 3, UNIT, ACCS),
    ("cat 32+96 3x3", 2, 64, 128, 32, 96, 8, 8, 3, UNIT, ACCS),
    ("cat 64+32 1x1", 2, 64, 96, 64, 32, 8, 8, 1, UNIT, ACCS),
    ("cat 128+128 1x1", 2, 128, 256, 128, 128, 8, 8, 1, UNIT, ACCS),
    ("cat 32+96 1x1", 2, 64, 128, 32, 96, 8, 8, 1, UNIT, ACCS),
    # one bench-sized launch per large-batch kernel (warp-specialised, ping-pong, small-level, 1x1 ping-pong)
    ("big 128->128 32x32", 64, 128, 128, 128, 0, 32, 32, 3, UNIT, ["raw"]),
    ("big 256->64 32x32", 64, 64, 256, 256, 0, 32, 32, 3, UNIT, ["raw"]),
    ("big 256->128 8x8", 255, 128, 256, 256, 0, 8, 8, 3, UNIT, ["raw"]),
    ("big 1x1 256->256 16x16", 128, 256, 256, 256, 0, 16, 16, 1, UNIT, ["raw"]),
]

# csrc/ops.h ConvKernel
K_IGEMM, K_1X1, K_1X1_PP, K_IN, K_OUT, K_PP, K_WS, K_SMALL = range(8)
KERNEL_NAMES = ["igemm", "1x1", "1x1_pp", "in", "out", "pp", "ws", "small"]
# every kernel a bias-free NHWC unit-mode conv can be routed to (the first-conv and last-conv kernels need a real input of <= 8 channels /
# an NCHW output); all of them exist for both element types of the backward pass: no exception is documented
WANT_KERNELS = {K_IGEMM, K_1X1, K_1X1_PP, K_PP, K_WS, K_SMALL}


def chunk(dtype_code):
    return 16 if dtype_code == 0 else 32
