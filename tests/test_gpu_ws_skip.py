"""GPU: a ResBlock's 1x1 skip_connection carried by the warp-specialised 3x3 conv (csrc/conv_ws.inc.h, SKIP instantiations; conv_ws bit 1).

At the levels whose second conv carries the GroupNorm + SiLU prologue (images at least 16 wide) `return skip_connection(x) + out_layers(h)`
(unet.py:312-317, 351) is one accumulation: a skip chunk is one more row item of the kernel's stream - one slot of the weight-row ring (its 8 KB
weight tile + the 16 x 16 interior pixels of one 64-byte chunk of the raw block input), of which the consumers multiply the centre tap only.  Items
travel in pairs behind pairs of kernel rows (`ws::skip_pairs`: item pairs rp np / nrp .. (rp + 1) np / nrp - 1 behind row pair rp, the last row pair
takes the rest); an odd chunk count is padded with an all-zero item.  Every case is checked through the C-ABI test op (mi355_conv2d_ex) against an fp64 CPU reference, against the
two-launch form of the same description (bit off: the 1x1 conv writes s, the 3x3 conv reads it as its residual), on the finalized GroupNorm partial
sums of its output, and for bit-identical repeats; a launch whose bounded counter wait expired fails the op (MI355_ERR_TIMEOUT), so every returned
tensor also says that the error word stayed zero.
"""
import pytest
import torch
import torch.nn.functional as F

from mi355 import _lib
from mi355._lib import MI355BackendError
from mi355.synth import randn, synth_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K_WS = 6
F32, BF16, F16 = _lib.MI355_F32, _lib.MI355_BF16, _lib.MI355_F16
# the tolerances of tests/test_gpu_configs.py (SMALL_FUSED_CASES / PP_CASES), as fractions of the reference's scale; U = unit roundoff of the stored type
DTYPES = [(F32, 5e-5, 0.0), (BF16, 3e-2, 2.0 ** -8), (F16, 4e-3, 2.0 ** -11)]
# conv_ws: bit 0 the kernel, bit 1 the carried skip conv, bit 2 launches with fewer tiles than CUs too, bits 8.. a workgroup limit.
# conv_pp = 0 / conv_min_wgs = 1: the plain geometry keeps the 128 x 128 tile the persistent kernel starts from, at any batch.
ON, OFF = 7, 5

CASES = [
    # B, C, H, W, Co, skip (c0, c1), workgroup limit
    (3, 128, 32, 32, 128, (128, 128), 0),   # four tiles per image, two skip sources of equal size: eight skip items (bf16) = four pairs over six row pairs
    (2, 128, 32, 32, 128, (256, 128), 0),   # the 384-channel block: one item pair behind every row pair (bf16), the source changes between pairs
    (3, 128, 16, 16, 128, (64, 0), 0),      # one tile per image; one item pair (bf16): only the tile's last row pair has one
    (2, 128, 24, 40, 128, (128, 128), 0),   # ragged 24 x 40: partial tiles in x and y, skip pixels outside the image are zero-filled by the DMA
    (2, 256, 32, 32, 128, (32, 0), 0),      # eight main chunks, ONE skip chunk (bf16): padded to a pair with the all-zero item
    (3, 128, 32, 32, 128, (256, 128), 5),   # 12 tiles on 5 workgroups: the stream crosses tile and image boundaries, uneven walks
    (2, 128, 16, 16, 256, (128, 0), 3),     # two 128-channel tiles per pixel tile: the second one's weights sit behind the first one's skip tiles
]


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def knobs(ws, limit=0):
    return _lib.debug_config(conv_ws=ws | (limit << 8), conv_pp=0, conv_min_wgs=1)


_REF = {}


def reference(case):
    """fp64 on the CPU, once per case: conv2d(silu(gn(h)), w3) + b3 + emb + conv2d(cat(x0, x1), w1) + b1, and s = the 1x1 part alone."""
    if case in _REF:
        return _REF[case]
    B, C, H, W, Co, (c0, c1), _ = case
    seed = 12000 + 17 * CASES.index(case)
    h = randn(seed, B, C, H, W) * 1.2 + 0.3
    x0 = randn(seed + 1, B, c0, H, W) * 1.1 + 0.1
    x1 = randn(seed + 2, B, c1, H, W) * 0.6 - 0.2 if c1 else None
    sd = synth_state_dict({"weight": (Co, C, 3, 3), "bias": (Co,)}, seed + 3)
    sw = synth_state_dict({"weight": (Co, c0 + c1, 1, 1), "bias": (Co,)}, seed + 4)
    g = synth_state_dict({"weight": (C,), "bias": (C,)}, seed + 5)
    gamma, beta = g["weight"] + 1.0, g["bias"]
    emb = randn(seed + 6, B, Co) * 0.5
    d = torch.float64
    act = F.silu(F.group_norm(h.to(d), 32, gamma.to(d), beta.to(d), eps=1e-5))
    main = F.conv2d(act, sd["weight"].to(d), sd["bias"].to(d), padding=1) + emb.to(d)[:, :, None, None]
    xs = x0 if x1 is None else torch.cat((x0, x1), 1)
    s = F.conv2d(xs.to(d), sw["weight"].to(d), sw["bias"].to(d))
    _REF[case] = dict(h=h, x0=x0, x1=x1, sd=sd, sw=sw, gamma=gamma, beta=beta, emb=emb, ref=main + s, s=s)
    return _REF[case]


def case_id(c):
    return "B{}_C{}_{}x{}_Co{}_skip{}+{}{}".format(c[0], c[1], c[2], c[3], c[4], c[5][0], c[5][1], f"_wg{c[6]}" if c[6] else "")


@pytest.mark.parametrize("case", CASES, ids=case_id)
@pytest.mark.parametrize("dtype,tol,u", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_carried_skip_conv(ops, case, dtype, tol, u):
    B, C, H, W, Co, (c0, c1), limit = case
    r = reference(case)
    ref, s_ref = r["ref"], r["s"]
    scale = ref.abs().max().item()
    gn = (r["gamma"].to(DEV), r["beta"].to(DEV))
    x1d = r["x1"].to(DEV) if r["x1"] is not None else None
    sk = (r["x0"].to(DEV), x1d, r["sw"]["weight"], r["sw"]["bias"])

    def fused():
        st = {}
        y, _, done = ops.conv2d_ex(r["h"].to(DEV), r["sd"]["weight"], r["sd"]["bias"], dtype=dtype, skip=sk, gn=gn, gn_silu=True, emb=r["emb"].to(DEV),
                                   stats=st, debug=knobs(ON, limit))
        return y.cpu(), done, st

    y, done, st = fused()
    assert done, "the launch did not carry the skip conv"
    assert (st["kernel"], st["tile_m"], st["tile_n"]) == (K_WS, 256, 128), st
    # (a) against the reference
    err = (y.double() - ref).abs().max().item()
    print(f"   WSSKIP {case_id(case)} dtype {dtype}: max err {err:.3e} = {err / scale:.2e} of scale {scale:.3f}")
    assert torch.isfinite(y).all()
    assert err < tol * scale
    # (b) the same description with the bit off: the op declines to carry it, the two convs run on their own (s stored in the element type)
    with pytest.raises(MI355BackendError):
        ops.conv2d_ex(r["h"].to(DEV), r["sd"]["weight"], r["sd"]["bias"], dtype=dtype, skip=sk, gn=gn, gn_silu=True, emb=r["emb"].to(DEV),
                      debug=knobs(OFF, limit))
    s = ops.conv2d(r["x0"].to(DEV), r["sw"]["weight"], r["sw"]["bias"], dtype=dtype, x1=x1d, debug=knobs(OFF, limit))
    info = {}
    two = ops.conv2d(r["h"].to(DEV), r["sd"]["weight"], r["sd"]["bias"], gn=gn, gn_silu=True, dtype=dtype, emb=r["emb"].to(DEV), res=s, res_mode=1,
                     debug=knobs(OFF, limit), info=info).cpu()
    assert info["kernel"] == K_WS, info
    # 16-bit types: s is rounded once when stored (<= u |s|) and either output once (<= u |y| each); fp32: the two sums differ in order only,
    # which the project's fp32 tolerance covers
    gap = (y.double() - two.double()).abs().max().item()
    bound = tol * scale if dtype == F32 else u * s_ref.abs().max().item() + 2 * u * scale + 5e-5 * scale
    print(f"   WSSKIP {case_id(case)} dtype {dtype}: fused vs two launches {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound
    # (c) the launch's own GroupNorm partial sums, finalized with gamma = 1, beta = 0 (a = rstd, b = -mean rstd), against fp64 statistics of the
    # reference.  The tensor may be off by e = tol * scale per element, so a group's mean by e and its variance by 2 sigma e + e^2.
    slots = 2 * ((W + 15) // 16) * ((H + 15) // 16)
    assert st["slots"] == slots, st["slots"]
    a, b = st["a"].cpu().double(), st["b"].cpu().double()
    grp = ref.reshape(B, 32, -1)
    mean, var = grp.mean(dim=2), grp.var(dim=2, unbiased=False)
    cpg = Co // 32
    mean_c, var_c = mean.repeat_interleave(cpg, dim=1), var.repeat_interleave(cpg, dim=1)
    e = tol * scale
    sig = var_c.sqrt()
    got_mean, got_var = -b / a, 1.0 / (a * a) - 1e-5
    dm = ((got_mean - mean_c).abs() - e).max().item()
    dv = ((got_var - var_c).abs() - (2 * sig * e + e * e) - 1e-5 * var_c).max().item()
    print(f"   WSSKIP {case_id(case)} dtype {dtype}: statistics beyond their budget: mean {dm:.3e} var {dv:.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert dm <= 0 and dv <= 0
    # ... and against fp64 statistics of the tensor the launch STORED, which is what bites in the 16-bit modes (a dropped slot moves a variance
    # by 1 / slots of itself).  The epilogue sums the fp32 accumulators v, the stored tensor is fl(v): the budget of tests/test_gpu_gn_ops.py
    # (rounding_gap; n elements per group, r = |mean| / sigma, six standard deviations of a mean of independent roundings <= u |v|):
    #   |dmean| <= 6 u sigma sqrt((1 + r^2) / (3 n)),  |dvar| <= 12 u sigma^2 sqrt((1 + r^2) / (3 n)) + u^2 sigma^2 (1 + r^2)
    # plus the fp32 partial sums themselves: a lane adds ~32 values and the slots meet in a tree, ~64 roundings deep = 4e-6 of rms(v) (of
    # rms(v)^2 for the sum of squares, twice for the difference), budgeted at 1e-5 rms(v) and 2e-5 rms(v)^2.
    ys = y.double().reshape(B, 32, -1)
    n = ys.shape[2]
    m_s, v_s = ys.mean(dim=2).repeat_interleave(cpg, dim=1), ys.var(dim=2, unbiased=False).repeat_interleave(cpg, dim=1)
    ms2 = v_s + m_s * m_s
    q = torch.sqrt(ms2 / (3 * n))                       # sigma sqrt((1 + r^2) / (3 n))
    dm2 = ((got_mean - m_s).abs() - (6 * u * q + 1e-5 * ms2.sqrt())).max().item()
    dv2 = ((got_var - v_s).abs() - (12 * u * v_s.sqrt() * q + u * u * ms2 + 2e-5 * ms2)).max().item()
    print(f"   WSSKIP {case_id(case)} dtype {dtype}: statistics vs the stored tensor beyond their budget: mean {dm2:.3e} var {dv2:.3e}")
    assert dm2 <= 0 and dv2 <= 0
    # (e) a second identical launch
    y2, _, _ = fused()
    assert torch.equal(y, y2)


def test_carried_skip_conv_in_network():
    """CIFAR net at B = 4, bit on against bit off (the persistent kernel forced for the small batch in both, the ping-pong kernel where its shapes
    are eligible, so that the 16x16 blocks keep their two launches in both): fp32 to the on / off tolerance of tests/test_gpu_upsample_phase.py,
    bf16 / fp16 not farther from the fp32 result than with the bit off by more than that file's spread, exactly three launches fewer (the skip
    convs of the three 32x32 output blocks)."""
    from image_diffusion.unet import UNetModel, param_shapes

    kw = dict(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,),
              channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64)
    sd = None
    B = 4

    def run(precision, ws):
        nonlocal sd
        net = UNetModel(precision=precision, **kw)
        if sd is None:
            sd = synth_state_dict(param_shapes(net), 9701)
        net.load_state_dict(sd)
        net.debug = _lib.debug_config(conv_ws=ws, conv_pp=47 | 64, conv_min_wgs=1)
        net.to(DEV)
        x = randn(9700, B, 3, 32, 32).to(DEV)
        t = torch.linspace(0, 1, B).to(DEV)
        e = net.engine(DEV)
        y = e.forward(x, t).cpu()
        torch.cuda.synchronize(); e.check()
        return y, e.stats(B)["launches"]

    on, l_on = run("fp32", ON)
    off, l_off = run("fp32", OFF)
    assert torch.isfinite(on).all()
    assert l_off - l_on == 3, (l_on, l_off)
    print(f"   WSSKIPNET fp32 max|on - off| {float((on - off).abs().max()):.3e} scale {float(off.abs().max()):.3f}")
    torch.testing.assert_close(on, off, rtol=2e-4, atol=2e-4)
    for prec in ("bf16", "fp16"):
        a, la = run(prec, ON)
        b, lb = run(prec, OFF)
        assert lb - la == 3, (prec, la, lb)
        scale = off.abs().max().item()
        ea, eb = (a - off).pow(2).mean().sqrt().item(), (b - off).pow(2).mean().sqrt().item()
        print(f"   WSSKIPNET {prec}: rms error vs fp32 on {ea:.4e} off {eb:.4e} scale {scale:.3f}")
        assert ea < 0.02 * scale and ea < 1.5 * eb + 1e-3 * scale, (prec, ea, eb, scale)
