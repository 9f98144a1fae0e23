"""CPU: the forward-conv reference of tests/conv_fwd_ref.py IS the operation (fp64, against independent F.conv2d compositions and the oracle's
ResBlock), its budget holds what it claims (fp32 eager's own error inside C_SUM / 4; a plain-torch emulation of a correct 16-bit kernel inside the
budget, and outside it with a truncating store, one dropped tap or a bias shifted by a channel), and conv_route sends every row of the table to the
kernel family, form and tile the row names (mi355_conv2d_fwd's route query: host code, no GPU).

Measured here (the FWDCPU lines): fp32 eager's own error reaches 5.67 x 2^-24 x mag over the table (the qkv 1x1 conv at 16x16), so C_SUM = 4 x 5.67 -> 23; the 16-bit emulation's worst
err / budget is 0.986 (bf16), 0.979 (fp16) and 0.981 (bf16x2) - a rounded store of an exact sum alone is 1 / 1.01 - and 0.79 / 0.79 / 0.71 over
the SiLU-prologue rows, whose six-sigma term is the statistical one.  The phase rows are also held as a phase launch is (phase=True: the emulated
phase packer, the mean checks against fp64 on the pre-summed filter): 0.27 ... 0.41 element-wise, and a truncating store fails their mean check at
4.1 ... 5.6 x six sigma.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from mi355.synth import randn
from tests import conv_fwd_ref as R
from tests.conv_fwd_ref import CASES, H16, KERNEL_NAMES


def _case(**kw):
    c = dict(idx=900, name="adhoc", B=2, cin=8, c1=0, cout=5, h=6, w=7, k=3, s=1, up=0, bias=1, pro=None, emb=0, res=0, nchw=0, axpy=0)
    c.update(kw)
    return c


@pytest.mark.parametrize("kw", [dict(), dict(k=1), dict(s=2), dict(s=2, h=7, w=7), dict(up=1), dict(c1=8), dict(pro="silu"), dict(pro="affine"),
                                dict(pro="silu", up=1, emb=1), dict(emb=1, res=1), dict(res=2, h=6, w=8), dict(pro="silu", c1=16, emb=1, res=1),
                                dict(cout=3, pro="silu", axpy=1)], ids=lambda kw: "_".join(f"{k}{v}" for k, v in kw.items()) or "plain")
def test_reference_is_the_operation(kw):
    """want against a composition written without the module's helpers: explicit zero padding after P, repeat_interleave for nearest x2, x sigmoid(x)."""
    c = _case(**kw)
    o = R.operands(c, "fp32")
    r = R.reference(c, o)
    x = torch.cat([o["x"]] + ([o["x1"]] if o["x1"] is not None else []), 1).double()
    if c["pro"]:
        v = o["a"].double()[:, :, None, None] * x + o["b"].double()[:, :, None, None]
        x = v * torch.sigmoid(v) if c["pro"] == "silu" else v
    if c["up"]:
        x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    p = c["k"] // 2
    y = F.conv2d(F.pad(x, (p, p, p, p)), o["W64"], stride=c["s"]) + o["bias"].double()[None, :, None, None]
    if c["emb"]:
        y = y + o["emb"].double()[:, :, None, None]
    if c["res"]:
        rr = o["res"].double()
        y = y + (rr.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3) if c["res"] == 2 else rr)
    if c["axpy"]:
        y = o["axpy_x"].double() + float(torch.tensor(o["axpy_s"], dtype=torch.float32)) * y
    assert tuple(r["want"].shape) == (c["B"], c["cout"]) + R.out_size(c)
    assert float((r["want"] - y).abs().max()) <= 1e-12 * float(y.abs().max())
    assert bool((r["mag"] >= r["want"].abs() * (1 - 1e-12)).all()), "mag bounds |want|"
    assert float((r["f32"].double() - y).abs().max()) <= 1e-4 * float(y.abs().max())
    if not c["pro"]:
        assert bool((r["cabs"] <= r["mag"] * (1 + 1e-12)).all())


def test_reference_composes_to_the_oracle_resblock():
    """Two reference convs with (a, b) taken from GroupNorm32 are the oracle's ResBlock(up=True) (oracle/unet_ref.py res_block): SiLU prologue, nearest
    x2 in the gather, emb, and the nearest-x2 residual."""
    from oracle.unet_ref import res_block

    B, Cc, h, w = 2, 64, 4, 4
    x = randn(501, B, Cc, h, w).double()
    sd = {"b.in_layers.0.weight": 1 + 0.1 * randn(502, Cc), "b.in_layers.0.bias": 0.1 * randn(503, Cc),      # fp32: group_norm32 runs in fp32
          "b.in_layers.2.weight": randn(504, Cc, Cc, 3, 3).double() / 24, "b.in_layers.2.bias": randn(505, Cc).double(),
          "b.emb_layers.1.weight": randn(506, Cc, 16).double() / 4, "b.emb_layers.1.bias": randn(507, Cc).double(),
          "b.out_layers.0.weight": 1 + 0.1 * randn(508, Cc), "b.out_layers.0.bias": 0.1 * randn(509, Cc),
          "b.out_layers.3.weight": randn(510, Cc, Cc, 3, 3).double() / 24, "b.out_layers.3.bias": randn(511, Cc).double()}
    emb = randn(512, B, 16).double()
    want = res_block(sd, "b", x, emb, Cc, Cc, True, False, False)

    def affine(t, g, b):     # GroupNorm32 as the per-(image, channel) affine the conv's prologue is given
        tg = t.reshape(B, 32, -1)
        mean, var = tg.mean(dim=2), tg.var(dim=2, unbiased=False)
        rstd = (var + 1e-5).rsqrt().repeat_interleave(Cc // 32, dim=1)
        a = rstd * g.double()[None]
        return a, b.double()[None] - mean.repeat_interleave(Cc // 32, dim=1) * a

    def ref_conv(t, a, b, W, bias, up=0, emb_t=None, res=None, res_mode=0):
        c = _case(B=B, cin=Cc, cout=Cc, h=t.shape[2], w=t.shape[3], up=up, pro="silu", emb=int(emb_t is not None), res=res_mode)
        o = dict(x=t, x1=None, a=a, b=b, W64=W, bias=bias, emb=emb_t, res=res, axpy_x=None, axpy_s=0.0)
        return R.reference(c, o)["want"]

    a1, b1 = affine(x, sd["b.in_layers.0.weight"], sd["b.in_layers.0.bias"])
    e = F.linear(F.silu(emb), sd["b.emb_layers.1.weight"], sd["b.emb_layers.1.bias"])
    h1 = ref_conv(x, a1, b1, sd["b.in_layers.2.weight"], sd["b.in_layers.2.bias"], up=1, emb_t=e)
    a2, b2 = affine(h1, sd["b.out_layers.0.weight"], sd["b.out_layers.0.bias"])
    got = ref_conv(h1, a2, b2, sd["b.out_layers.3.weight"], sd["b.out_layers.3.bias"], res=x, res_mode=2)
    # the oracle's group_norm32 runs in fp32 (nn.py:87-94): its own rounding is the tolerance
    assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())


def test_phase_filters_are_the_nine_tap_conv():
    """phase_weights restates conv_pack_weights_up2.  With small-integer weights every sum is exact, so the four phase filters give the nine-tap conv
    of the up-sampled image exactly, ragged sizes and the zero padding included; and each filter has at most four non-zero taps (a 2x2 conv)."""
    Wt = (randn(601, 5, 3, 3, 3) * 3).round()
    x = F.interpolate((randn(602, 2, 3, 5, 7) * 4).round().double(), scale_factor=2, mode="nearest")
    for dt in ("fp32", "bf16", "fp16"):
        ph = R.phase_weights(Wt, dt)
        assert len(ph) == 4 and all(int((E != 0).sum(dim=(2, 3)).max()) <= 4 for E in ph)
        assert torch.equal(R._phase_conv(x, ph), F.conv2d(x, Wt.double(), padding=1))
    # one rounding of the sum, not the sum of the roundings
    Wr = randn(603, 4, 2, 3, 3)
    E = R.phase_weights(Wr, "bf16")[0]
    assert torch.equal(E[:, :, 1, 1], R.rnd(((Wr[:, :, 1, 1] + Wr[:, :, 1, 2]) + Wr[:, :, 2, 1]) + Wr[:, :, 2, 2], "bf16"))


def test_fp32_eager_error_is_inside_c_sum():
    """The budget's 4 x max|f32 - want| + C_SUM 2^-24 mag rests on fp32 eager's own error staying below C_SUM / 4 x 2^-24 x mag on this table."""
    worst, where = 0.0, None
    threads = torch.get_num_threads()
    torch.set_num_threads(1)      # eager's summation order follows its blocking: one thread makes the measured figure repeatable
    try:
        for c in CASES:
            if "fp32" not in c["types"]:
                continue
            o, r = R.case_data(c["idx"], "fp32")
            f32 = R._compose(c, o, torch.float32, o["W64"].float())
            e = (f32.double() - r["want"]).abs()
            if c["pro"] == "silu":       # eager rounds a v + b too: that part has the budget's own term
                e = (e - R.K_FMA * R.U32 * r["magpro"]).clamp_min(0.0)
            ratio = float((e / (R.U32 * r["mag"])).max())
            if ratio > worst:
                worst, where = ratio, c["name"]
    finally:
        torch.set_num_threads(threads)
    print(f"   FWDCPU fp32 eager worst |f32 - want| / (2^-24 mag) = {worst:.2f} ({where}); C_SUM / 4 = {R.C_SUM / 4}")
    assert worst <= R.C_SUM / 4, (worst, where)


@pytest.mark.parametrize("dt", ["bf16", "fp16", "bf16x2"])
def test_emulated_16bit_kernel_is_inside_the_budget(dt):
    """Rounding P to the type, multiplying in fp32 and rounding the store - the arithmetic of a correct kernel - passes every check of every row."""
    worst, where, worst_silu, where_silu = 0.0, None, 0.0, None
    for c in CASES:
        if dt not in c["types"]:
            continue
        o, r = R.case_data(c["idx"], dt)
        ratio = R.check(f"{dt} {c['name']} (emulation)", c, dt, R.emulate16(c, dt, o), r, phase=False, log=lambda s: None)
        if c["fam"] == R.K_PP and R.want_form(c, dt) == 2:     # the phase packer: the fp32 taps summed, rounded once; held as a phase launch is
            ratio = max(ratio, R.check(f"{dt} {c['name']} (phase emulation)", c, dt, R.emulate16(c, dt, o, phase=True), r, phase=True,
                                       log=lambda s: None))
        if ratio > worst:
            worst, where = ratio, c["name"]
        if c["pro"] == "silu" and ratio > worst_silu:
            worst_silu, where_silu = ratio, c["name"]
    print(f"   FWDCPU {dt} emulation worst err / budget {worst:.3f} ({where}); SiLU-prologue rows {worst_silu:.3f} ({where_silu})")
    assert worst < 1.0


# one row per family and epilogue kind, NHWC and NCHW outputs
DEFECT_ROWS = ["ig 128x128 64->128 16x16", "ig 64->64 20x28 silu", "1x1 qkv 128->384 8x8 affine", "pp1 256x256 256->256 16x16", "in 3->128 16x16",
               "pp wide silu 128->256 16x16", "pp phase 64->256 16x16", "pp phase 128->256 20x20 emb", "pp phase 192->512 16x16", "ws silu 128->128 16x16 res up2", "small 8x8 128->256 B3 emb res",
               "small 4x4 128->128 B5", "out 128->3 16x16", "out 128->3 16x16 axpy"]


@pytest.mark.parametrize("dt", H16)
@pytest.mark.parametrize("defect", ["trunc", "drop_tap", "shift_bias"])
def test_emulated_defects_fail(dt, defect):
    """The same emulation with a truncating 16-bit store, with tap (0, 0) of one input channel missing, and with the bias of the next channel: each
    must fail a check (truncation only exists where a 16-bit value is stored: the NHWC rows)."""
    by_name = {c["name"]: c for c in CASES}
    ran = 0
    for name in DEFECT_ROWS:
        c = by_name[name]
        if dt not in c["types"] or (defect == "trunc" and not R.nhwc_out(c)):
            continue
        o, r = R.case_data(c["idx"], dt)
        phase = c["fam"] == R.K_PP and R.want_form(c, dt) == 2      # held as the launch is: the phase packer's filter, the phase checks
        got = R.emulate16(c, dt, o, store="trunc" if defect == "trunc" else "round", drop_tap=defect == "drop_tap", shift_bias=defect == "shift_bias",
                          phase=phase)
        with pytest.raises(AssertionError):
            R.check(f"{dt} {name} ({defect})", c, dt, got, r, phase=phase, log=lambda s: None)
        ran += 1
    assert ran >= 8


def test_table_is_named_and_small():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert c["types"] and set(c["types"]) <= set(R.TYPES)
        assert set(c["types"]) >= set(R.ALL3) or c["why"], f"{c['name']}: a type is missing without a reason"
        big = c["fam"] == R.K_SMALL and R.EXPECT.get(c["name"], R.EXPECT_DEFAULT)[4] < 4     # the K split follows the launch size
        assert c["B"] <= 3 or big or R.out_size(c)[0] <= 4, f"{c['name']}: B = {c['B']}"     # 4x4 outputs: four images per tile, an odd batch


@pytest.fixture(scope="module")
def ops():
    import __graft_entry__ as ge

    ge.build()
    from mi355.ops import default_ops

    return default_ops


def test_route_table(ops):
    """conv_route over the whole table: each row's kernel family, form, tile and the remaining route words, per element type; and per type the set
    of (kernel, form) pairs is every ConvKernel value with every form its route function can produce (named exception: no fp32 first-conv kernel)."""
    for dt in R.TYPES:
        reached = {}
        for c in CASES:
            if dt not in c["types"]:
                continue
            got = ops_route(ops, c, dt)
            assert got == R.want_route(c, dt), f"{dt} {c['name']}: conv_route says {got}, the table {R.want_route(c, dt)}"
            reached.setdefault((got["kernel"], got["form"]), []).append(c["name"])
        print(f"   FWDROUTE {dt}: " + ", ".join(f"{KERNEL_NAMES[k]}/{f} x{len(v)}" for (k, f), v in sorted(reached.items())))
        if dt in R.ALL3:
            assert set(reached) == R.want_pairs(dt), f"{dt}: reached {sorted(reached)}, wanted {sorted(R.want_pairs(dt))}"
        else:   # split weights never leave the implicit-GEMM kernels (conv_route)
            assert set(reached) == {(R.K_IGEMM, 0)}


def ops_route(ops, c, dt):
    r = R.route_query(ops, c, dt)
    r.pop("n_mt")
    return r


def test_fwd_op_argument_checks(ops):
    from mi355 import _lib

    L = _lib.lib()
    route = (C.c_int32 * 8)()
    some = C.c_void_p(256)

    def q(batch, cin, cin1, cout, h, w, k, stride, resample, dtype, pro=False, emb=False, res_mode=0, flags=0, axpy=False):
        return L.mi355_conv2d_fwd(None, None, cin1, None, None, None, batch, cin, h, w, cout, k, stride, resample, some if pro else None,
                                  some if pro else None, 1, some if emb else None, some if res_mode else None, res_mode or 1, flags,
                                  some if axpy else None, 0.0, dtype, None, route, None, 0, None)

    F32, BF = _lib.MI355_F32, _lib.MI355_BF16
    assert q(2, 64, 0, 64, 8, 8, 3, 1, 0, F32) == 0 and route[0] >= 0 and route[2] > 0
    assert q(2, 128, 0, 3, 16, 16, 3, 1, 0, BF, pro=True) == 0 and route[0] == R.K_OUT     # the route is reported for the NCHW fp32 out conv too
    assert q(2, 64, 0, 64, 8, 8, 3, 1, 0, 7) < 0 and b"dtype" in L.mi355_last_error()
    assert list(route) == [-1] * 8
    assert q(2, 64, 0, 64, 8, 8, 5, 1, 0, F32) < 0 and b"kernel size" in L.mi355_last_error()
    assert q(2, 64, 0, 64, 8, 8, 3, 3, 0, F32) < 0 and b"stride" in L.mi355_last_error()
    assert q(2, 64, 0, 64, 8, 8, 3, 1, 3, F32) < 0 and b"pooling" in L.mi355_last_error()
    assert q(2, 64, 0, 64, 8, 8, 3, 2, 2, F32) < 0 and b"combined" in L.mi355_last_error()
    assert q(2, 64, 0, 64, 8, 8, 1, 2, 0, F32) < 0 and b"3x3" in L.mi355_last_error()
    assert q(2, 64, 0, 64, 8, 8, 3, 1, 0, F32, flags=2) < 0 and b"flag" in L.mi355_last_error()
    assert q(2, 64, 24, 64, 8, 8, 3, 1, 0, BF) < 0 and b"two-source" in L.mi355_last_error()
    assert q(2, 6, 3, 128, 16, 16, 3, 1, 0, BF, flags=1) < 0 and b"at most 8" in L.mi355_last_error()
    assert q(2, 48, 0, 64, 8, 8, 3, 1, 0, BF, pro=True) < 0 and b"prologue" in L.mi355_last_error()
    assert q(2, 128, 0, 3, 16, 16, 3, 1, 0, F32, emb=True) < 0 and b"NHWC" in L.mi355_last_error()
    assert q(2, 128, 0, 64, 16, 16, 3, 1, 0, F32, axpy=True) < 0 and b"Euler" in L.mi355_last_error()
    assert q(2, 64, 0, 64, 8, 8, 3, 1, 0, F32, res_mode=3) < 0 and b"res_mode" in L.mi355_last_error()
    # a launch needs its pointers: without a workspace and without a route there is nothing to do
    assert L.mi355_conv2d_fwd(None, None, 0, None, None, None, 2, 64, 8, 8, 64, 3, 1, 0, None, None, 0, None, None, 1, 0, None, 0.0, F32, None, None,
                              None, 0, None) < 0 and b"null argument" in L.mi355_last_error()
