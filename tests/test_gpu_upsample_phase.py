"""GPU: the phase form of the ping-pong 3x3 kernel (csrc/conv_pp.inc.h, UP = 1; conv_pp bit 6).

Upsample.conv (unet.py:209-212) is a 3x3 conv over F.interpolate(x, scale_factor=2, mode="nearest").  Neighbouring taps of the filter read the
same low-res pixel, so output phase (a, b) = (row parity, column parity) is a 2x2 conv of the low-res image with the filter rows / columns
summed: [w0, w1 + w2] for phase 0, [w0 + w1, w2] for phase 1 (conv_pack_weights_up2).  Every case is checked against the CPU reference, against
the nine-tap ping-pong path of the same op, and with the epilogue's counted wait window replaced by a drain (identical tensor); the op reports the
form it launched, so a case fails if the phase form silently did not run.
"""
import pytest
import torch
import torch.nn.functional as F

from mi355 import _lib
from mi355.synth import randn, synth_state_dict
from tests.test_gn_ref_cpu import make_params
from tests.test_gpu_gn_ops import U16, check_partial, class_bias, conv_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
K_PP, FORM_PHASE, FORM_WIDE = 5, 2, 0
F32, BF16, F16 = _lib.MI355_F32, _lib.MI355_BF16, _lib.MI355_F16
# the tolerances of tests/test_gpu_configs.py::test_pingpong_conv
DTYPES = [(F32, 5e-5, 5e-5), (BF16, 3e-2, 3e-2), (F16, 4e-3, 4e-3)]

CASES = [
    # N, C0, C1, low-res H, W, Cout, emb
    (3, 64, 0, 16, 16, 256, False),     # one tile per image and phase, fewer tiles than CUs
    (70, 64, 0, 16, 16, 256, False),    # 280 tiles on 256 CUs: the walk crosses phase and image boundaries, uneven walks, the DMA stream across tiles
    (2, 64, 64, 16, 16, 256, False),    # two-source concat
    (2, 64, 0, 20, 24, 256, False),     # ragged low-res tiles (masked pixels in the stores), non-square
    (2, 64, 0, 16, 16, 512, False),     # two channel tiles
    (2, 128, 0, 16, 16, 256, True),     # an emb row in the epilogue
]


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def reference(x, x1, w, b, emb):
    h = x if x1 is None else torch.cat((x, x1), dim=1)
    ref = F.conv2d(F.interpolate(h, scale_factor=2, mode="nearest"), w, b, padding=1)
    return ref if emb is None else ref + emb[:, :, None, None]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "N{}_C{}+{}_{}x{}_Co{}{}".format(*c[:6], "_emb" if c[6] else ""))
@pytest.mark.parametrize("dtype,rtol,atol", DTYPES, ids=["fp32", "bf16", "fp16"])
def test_phase_conv(ops, case, dtype, rtol, atol):
    """conv_pp = 2 | 64 against the CPU reference, against conv_pp = 2 (nine taps on the up-sampled gather), and with conv_ablate = 64."""
    N, C0, C1, H, W, Co, use_emb = case
    seed = 9100 + 17 * CASES.index(case)
    x = randn(seed, N, C0, H, W) * 1.3 + 0.1
    x1 = randn(seed + 1, N, C1, H, W) * 0.7 - 0.2 if C1 else None
    sd = synth_state_dict({"weight": (Co, C0 + C1, 3, 3), "bias": (Co,)}, seed + 2)
    emb = randn(seed + 3, N, Co) * 0.5 if use_emb else None
    ref = reference(x, x1, sd["weight"], sd["bias"], emb)

    def run(**knobs):
        info = {}
        y = ops.conv2d(x.to(DEV), sd["weight"], sd["bias"], resample=2, dtype=dtype, x1=x1.to(DEV) if x1 is not None else None,
                       emb=emb.to(DEV) if emb is not None else None, debug=_lib.debug_config(**knobs), info=info).cpu()
        return y, info

    got, info = run(conv_pp=2 | 64)
    assert (info["kernel"], info["form"]) == (K_PP, FORM_PHASE), f"the phase form did not run: {info}"
    assert (info["tile_m"], info["tile_n"]) == (256, 256), info
    drained, info_d = run(conv_pp=2 | 64, conv_ablate=64)
    assert (info_d["kernel"], info_d["form"]) == (K_PP, FORM_PHASE), info_d
    nine, info9 = run(conv_pp=2)
    assert (info9["kernel"], info9["form"]) == (K_PP, FORM_WIDE), f"the nine-tap ping-pong path did not run: {info9}"
    print(f"   PHASE case {case} dtype {dtype}: max|got - ref| {float((got - ref).abs().max()):.3e}  max|nine - ref| {float((nine - ref).abs().max()):.3e}"
          f"  max|got - nine| {float((got - nine).abs().max()):.3e}  scale {float(ref.abs().max()):.2f}")
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol)
    torch.testing.assert_close(got, nine, rtol=rtol, atol=atol)
    assert torch.equal(got, drained)


def test_phase_weight_table_exact(ops):
    """One non-zero low-res pixel, one non-zero tap (all channels but one zero as well): the inputs are powers of two, so every product is exact in fp32, and every output pixel
    has at most one term, so the result equals the reference bit for bit - for each of the nine taps; pins the tap -> (phase, 2x2 tap) table."""
    N, Ci, Co, H, W = 2, 64, 256, 16, 16
    for tap in range(9):
        x = torch.zeros(N, Ci, H, W)
        x[0, 5, 7, 9] = 2.0
        x[1, 40, 0, 15] = -0.5            # a corner-row pixel: the zero padding of both resolutions
        w = torch.zeros(Co, Ci, 3, 3)
        w[:, 5, tap // 3, tap % 3] = randn(9200 + tap, Co)
        w[:, 40, tap // 3, tap % 3] = randn(9300 + tap, Co)
        b = randn(9400, Co)
        ref = reference(x, None, w, b, None)
        info = {}
        got = ops.conv2d(x.to(DEV), w, b, resample=2, dtype=F32, debug=_lib.debug_config(conv_pp=2 | 64), info=info).cpu()
        assert (info["kernel"], info["form"]) == (K_PP, FORM_PHASE), info
        assert torch.equal(got, ref), f"tap {tap}: {int((got != ref).sum())} elements differ, max {float((got - ref).abs().max()):.3e}"


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("shape", [(3, 64, 16, 16, 256), (2, 64, 20, 24, 256)], ids=["16x16", "ragged20x24"])
def test_phase_conv_groupnorm_partials(ops, shape, dtype):
    """The GroupNorm partial sums of the phase form's epilogue, one slot per (phase, low-res tile, pixel wave), then gn_finalize: (a, b) against fp64
    GroupNorm of the tensor the conv stored, and that tensor against the CPU conv - the checks and budgets of
    tests/test_gpu_gn_ops.py::test_conv_partial_sums_and_finalize_vs_fp64.  Ragged tiles must count in-image pixels only.  The site against GroupNorm of the
    CPU conv result follows from the two: the budget of (a, b) is a few fp32 ulps of the statistics, far below what the conv's own tolerance moves them, so
    a direct comparison could only be made at the conv's tolerance and would see less."""
    N, Ci, H, W, Co = shape
    TORCH16 = {BF16: torch.bfloat16, F16: torch.float16}
    x = randn(9500, N, Ci, H, W)
    w = conv_weights(9501, Co, Ci, 3)
    bias = class_bias(9502, Co, Co, 0)
    worst = {}
    for film_on in (False, True):
        gamma, beta, film = make_params(9503, N, Co, film_on)
        tag = f"phase {H}x{W} dtype {dtype} film={film_on}"
        r = ops.conv2d_gn(x.to(DEV), w, bias, gamma.to(DEV), beta.to(DEV), film=film.to(DEV) if film is not None else None, resample=2, dtype=dtype,
                          debug=_lib.debug_config(conv_pp=2 | 64))
        assert (r["kernel"], r["form"]) == (K_PP, FORM_PHASE), f"{tag}: kernel {r['kernel']} form {r['form']}"
        assert r["slots"] == 4 * 2 * ((H + 15) // 16) * ((W + 15) // 16), f"{tag}: {r['slots']} slots"
        y = r["y"].cpu()
        xr, wr = (x, w) if dtype == F32 else (x.to(TORCH16[dtype]).float(), w.to(TORCH16[dtype]).float())
        want = F.conv2d(F.interpolate(xr.double(), scale_factor=2, mode="nearest"), wr.double(), bias.double(), padding=1)
        err = float((y.double() - want).abs().max())
        # the collapsed weights are rounded once AFTER the sum: against the reference with per-tap rounded weights a 16-bit run differs by up to one more
        # weight rounding per summed pair, inside the 2.5 u budget of the existing test (u = unit roundoff)
        tol = (1e-4 if dtype == F32 else 2.5 * U16[dtype]) * float(want.abs().max())
        print(f"   PHASEGN {tag}: conv err {err:.3e} tol {tol:.3e} slots {r['slots']}")
        assert err < tol, f"{tag}: conv output"
        check_partial(r, [y], gamma, beta, film, dtype, tag, worst)


def test_phase_form_in_network():
    """CIFAR net at B = 4, phase form forced on (conv_pp 47 | 64) against forced off (47): fp32 to the golden tolerance of tests/test_gpu_unet.py, bf16 /
    fp16 not farther from the fp32 result than the forced-off run, equal launch counts."""
    from image_diffusion.unet import UNetModel, param_shapes

    kw = dict(image_size=32, in_channels=3, model_channels=128, out_channels=3, num_res_blocks=2, attention_resolutions=(2,),
              channel_mult=(1, 2, 2, 2), num_heads=4, num_head_channels=64)
    sd = None
    B = 4

    def run(precision, **knobs):
        nonlocal sd
        net = UNetModel(precision=precision, **kw)
        if sd is None:
            sd = synth_state_dict(param_shapes(net), 9601)
        net.load_state_dict(sd)
        net.debug = _lib.debug_config(**knobs)
        net.to(DEV)
        x = randn(9600, B, 3, 32, 32).to(DEV)
        t = torch.linspace(0, 1, B).to(DEV)
        e = net.engine(DEV)
        y = e.forward(x, t).cpu()
        torch.cuda.synchronize(); e.check()
        return y, e.stats(B)["launches"]

    on, l_on = run("fp32", conv_pp=47 | 64)
    off, l_off = run("fp32", conv_pp=47)
    assert torch.isfinite(on).all()
    assert l_on == l_off, (l_on, l_off)
    assert not torch.equal(on, off), "forced on and forced off gave the same bits: the phase form did not run in the network"
    print(f"   PHASENET fp32 max|on - off| {float((on - off).abs().max()):.3e} scale {float(off.abs().max()):.3f}")
    torch.testing.assert_close(on, off, rtol=2e-4, atol=2e-4)
    for prec in ("bf16", "fp16"):
        a, la = run(prec, conv_pp=47 | 64)
        b, lb = run(prec, conv_pp=47)
        assert la == lb, (prec, la, lb)
        scale = off.abs().max().item()
        ea, eb = (a - off).pow(2).mean().sqrt().item(), (b - off).pow(2).mean().sqrt().item()
        print(f"   PHASENET {prec}: rms error vs fp32 on {ea:.4e} off {eb:.4e} scale {scale:.3f}")
        assert ea < 0.02 * scale and ea < 1.5 * eb + 1e-3 * scale, (prec, ea, eb, scale)
