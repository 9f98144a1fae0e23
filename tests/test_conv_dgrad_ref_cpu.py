"""CPU: the conv data gradient as the U-Net backward decomposes it IS the gradient (fp64, against autograd), and the GPU test's shape table
reaches every conv kernel the data gradient can be routed to.

The decomposition (tests/conv_dgrad_ref.py dgrad_decomposed; csrc/unet_backward.hip conv_dgrad_launch): transposed, tap-flipped filter; zero
insertion for stride 2; one stride-1 conv; 2x2 block sums for nearest x2; zero channels up to cin_pad; the split at c0.  This guards the reference
of tests/test_gpu_conv_dgrad.py and the maths, not the kernels; conv_route is host code, so the route table is checked here as well.
"""
import pytest
import torch

from mi355.synth import randn
from tests.conv_dgrad_ref import (CASES, KERNEL_NAMES, STRIDE2, UNIT, UP2, WANT_KERNELS, chunk, cin_pad_of, dgrad_autograd, dgrad_decomposed,
                                  out_size)

# (h, w, mode): the stride-2 sizes are 7x7 -> 4x4 (odd: the last input row is a stuffed position) and 8x6 -> 4x3 (even: a trailing zero row)
SIZES = [(4, 4, UNIT), (7, 5, UNIT), (8, 8, UNIT), (7, 7, STRIDE2), (8, 6, STRIDE2), (4, 4, UP2), (7, 5, UP2)]
# (Ci, c0, c1): one source and two; Ci = 1, 3, 6 inside a padded chunk of 16; a padded first source is never followed by a second one
CHANNELS = [(1, 16, 0), (3, 16, 0), (6, 16, 0), (32, 32, 0), (24, 16, 8), (40, 8, 32)]


# the resampling convs of the network are 3x3: k = 1 goes with the plain mode only
@pytest.mark.parametrize("k,h,w,mode", [(k, h, w, m) for k in (1, 3) for (h, w, m) in SIZES if k == 3 or m == UNIT])
def test_decomposition_is_the_gradient(k, h, w, mode):
    Ho, Wo = out_size(h, w, mode)
    for ci, (Ci, c0, c1) in enumerate(CHANNELS):
        for Co in (5, 32):
            B = 2
            seed = 1000 * k + 100 * h + 10 * w + mode
            W = randn(91000 + seed + ci, Co, Ci, k, k).double()
            G = randn(92000 + seed + ci, B, Co, Ho, Wo).double()
            a0, a1, hi = dgrad_autograd(W, G, c0, c1, h, w, mode, with_hi=True)
            d0, d1, raw = dgrad_decomposed(W, G, c0, c1, h, w, mode)
            tag = f"k={k} {h}x{w} mode={mode} Ci={Ci} c0={c0} c1={c1} Co={Co}"
            scale = float(a0.abs().max())
            assert scale > 0, tag
            assert float((d0 - a0).abs().max()) <= 1e-12 * scale, tag
            if c1:
                assert float((d1 - a1).abs().max()) <= 1e-12 * float(a1.abs().max()), tag
            assert raw.shape[1] == cin_pad_of(c0, c1) and torch.equal(raw[:, Ci:], torch.zeros_like(raw[:, Ci:])), tag
            assert torch.equal(raw[:, :c0], d0) and (not c1 or torch.equal(raw[:, c0:c0 + c1], d1)), tag
            both = torch.cat([a0] + ([a1] if c1 else []), dim=1)
            assert torch.equal(both[:, Ci:], torch.zeros_like(both[:, Ci:])), f"{tag}: padding channels of the reference"
            if mode == UP2:     # the intermediate the bf16 budget of the GPU test is taken over
                assert float((hi.reshape(B, Ci, h, 2, w, 2).sum(dim=(3, 5)) - both[:, :Ci]).abs().max()) <= 1e-12 * scale, tag


def test_stride2_stuffed_positions():
    """Odd and even inputs: which input rows and columns an output gradient lands on (2 y, 2 x) and which stay without a centre tap."""
    for h, w in ((7, 7), (8, 6), (8, 8), (5, 4)):
        Ho, Wo = out_size(h, w, STRIDE2)
        W = torch.zeros(1, 1, 3, 3, dtype=torch.float64)
        W[0, 0, 1, 1] = 1.0                                   # centre tap only: the gradient is the zero-stuffed G itself
        G = randn(93000 + h, 1, 1, Ho, Wo).double()
        a0, _ = dgrad_autograd(W, G, 8, 0, h, w, STRIDE2)
        want = torch.zeros(1, 8, h, w, dtype=torch.float64)
        want[:, :1, 0:2 * Ho:2, 0:2 * Wo:2] = G
        assert torch.equal(a0, want)
        assert torch.equal(dgrad_decomposed(W, G, 8, 0, h, w, STRIDE2)[0], want)


def test_route_table_reaches_every_kernel():
    """conv_route over the GPU test's table (mi355_conv2d_vjp without a workspace: host code only).  A retuned router that no longer sends any
    of these shapes to one of the kernels fails here, before the GPU test's own coverage assertion."""
    import __graft_entry__ as ge

    ge.build()
    from mi355 import _lib
    from mi355.ops import default_ops as ops

    for dtype, name in ((_lib.MI355_F32, "fp32"), (_lib.MI355_BF16, "bf16")):
        reached = {}
        for (cname, B, Co, Ci, c0, c1, h, w, k, mode, forms) in CASES:
            r = ops.conv2d_vjp_route(B, Co, Ci, c0 if c0 is not None else chunk(dtype), c1, h, w, k, mode, dtype=dtype)
            reached.setdefault(r["kernel"], []).append(cname)
        for kk, names in sorted(reached.items()):
            print(f"   DGRADROUTE {name} {KERNEL_NAMES[kk]}: {len(names)} cases, e.g. {names[0]}")
        assert set(reached) >= WANT_KERNELS, f"{name}: reached {sorted(KERNEL_NAMES[x] for x in reached)}"


def test_vjp_op_argument_checks():
    import ctypes as C

    from mi355 import _lib

    L = _lib.lib()
    route = (C.c_int32 * 4)()
    q = lambda *a: L.mi355_conv2d_vjp(None, None, None, None, None, 0, 0, *a, None, route, None, 0, None)
    # batch, cout, cin, c0, c1, h, w, ksize, mode, g_channels, dtype
    assert q(2, 64, 64, 64, 0, 8, 8, 3, 0, 64, _lib.MI355_F32) == 0 and route[0] >= 0
    assert q(2, 64, 64, 32, 0, 8, 8, 3, 0, 64, _lib.MI355_F32) < 0 and b"c0 + c1" in L.mi355_last_error()
    assert q(2, 64, 64, 64, 0, 8, 8, 1, 1, 64, _lib.MI355_F32) < 0 and b"3x3" in L.mi355_last_error()
    assert q(2, 3, 64, 64, 0, 8, 8, 3, 0, 16, _lib.MI355_BF16) < 0 and b"g_channels" in L.mi355_last_error()
    assert q(2, 64, 60, 60, 0, 8, 8, 3, 0, 64, _lib.MI355_BF16) < 0 and b"fragments" in L.mi355_last_error()
    assert list(route) == [-1, -1, -1, -1]
