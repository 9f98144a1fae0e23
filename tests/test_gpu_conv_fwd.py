"""GPU: one forward convolution as the network launches it, op by op, against fp64 on the values the kernel reads.

mi355_conv2d_fwd builds the ConvDesc the engine builds - prologue (a, b) given directly, second source, emb, residual, stride 2 / nearest x2, the
first conv's NCHW read and the out conv's Euler update - and calls conv_route / conv_launch.  Reference, budget and the table of named rows:
tests/conv_fwd_ref.py (held to the maths, to an emulation of a correct 16-bit kernel and to conv_route on the CPU by tests/test_conv_fwd_ref_cpu.py).
Every call fills the op's workspace with 0xFF bytes and the output with NaN: an element no kernel writes fails the finiteness check.  Each row asserts
the launched (kernel, form, tile, reads_nchw, axpy, ksplit) against the row's expected values and against the route query; the ping-pong 3x3 rows are
launched a second time with conv_ablate = 64 (the counted epilogue window replaced by a drain), which must give the same bits.  A phase-form launch has its per-channel mean checks taken against fp64 on the pre-summed filter it reads (conv_fwd_ref.py
phase_weights), and a row with axpy_x asserts that the tensor the launch did not write is untouched.

Measured on the MI355X (worst err / budget over all rows, the FWDSUM lines; DESIGN.md section 8c has the table per family): fp32 0.847 (ping-pong
3x3, wide, SiLU prologue, 192 -> 256 at 28x28), bf16 0.986, fp16 0.979, bf16x2 0.981 (a correctly rounded 16-bit store of an exact value alone
measures 1 / 1.01 of its term; the CPU emulation of a correct kernel gives the same three figures).  The 335 parametrisations take 8 s.
"""
import pytest
import torch

from mi355 import _lib
from tests import conv_fwd_ref as R
from tests.conv_fwd_ref import CASES, KERNEL_NAMES

DEV = "cuda:0"
RUN_TYPES = ("fp32", "bf16", "fp16")          # bf16x2 rows run with bf16's closing test
REACHED = {dt: {} for dt in R.TYPES}          # case index -> (kernel, form) the launch reported
WORST = {dt: {} for dt in R.TYPES}            # case index -> worst err / budget


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def _launch(ops, c, dt, o, knobs, info):
    d = lambda t: t.to(DEV) if t is not None else None
    return ops.conv2d_fwd(d(o["x"]), o["W"], o["bias"], stride=c["s"], resample=2 if c["up"] else 0,
                          pro=(d(o["a"]), d(o["b"])) if c["pro"] else None, pro_silu=c["pro"] == "silu", dtype=R.dtype_code(dt), x1=d(o["x1"]),
                          emb=d(o["emb"]), res=d(o["res"]), res_mode=c["res"] or 1, nchw_src=bool(c["nchw"]), axpy_x=d(o["axpy_x"]),
                          axpy_scale=o["axpy_s"], debug=_lib.debug_config(**knobs), ws_fill=0xFF, info=info)


def run_case(ops, dt, idx):
    c = CASES[idx]
    o, r = R.case_data(idx, dt)
    info = {}
    got = _launch(ops, c, dt, o, c["knobs"], info)
    info.pop("n_mt")
    y, xu = info.pop("y"), info.pop("axpy_x")
    if c["axpy"]:     # exactly one of the two is written: the Euler update replaces the store, or the store leaves axpy_x alone
        if info["axpy"]:
            assert bool(torch.isnan(y).all()), f"{dt} {c['name']}: the Euler update replaced the store, yet {int((~torch.isnan(y)).sum())} elements of y were written"
        else:
            assert torch.equal(xu.cpu(), o["axpy_x"]), f"{dt} {c['name']}: v was stored to y, yet axpy_x changed"
    tag = f"{dt} {c['name']} B={c['B']} [{KERNEL_NAMES[info['kernel']]} form {info['form']} {info['tile_m']}x{info['tile_n']}]"
    assert info == R.want_route(c, dt), f"{tag}: launched {info}, the table says {R.want_route(c, dt)}"
    q = R.route_query(ops, c, dt)
    q.pop("n_mt")
    assert info == q, f"{tag}: launched {info}, conv_route says {q}"
    worst = R.check(tag, c, dt, got, r, phase=info["kernel"] == R.K_PP and info["form"] == 2)
    if info["kernel"] == R.K_PP:
        info2 = {}
        drained = _launch(ops, c, dt, o, dict(c["knobs"], conv_ablate=64), info2)
        assert info2["kernel"] == R.K_PP and info2["form"] == info["form"]
        assert torch.equal(drained, got), f"{tag}: conv_ablate = 64 changes {int((drained != got).sum())} elements"
    REACHED[dt][idx] = (info["kernel"], info["form"])
    WORST[dt][idx] = worst


PARAMS = [(dt, c["idx"]) for c in CASES for dt in c["types"]]


@pytest.mark.gpu
@pytest.mark.parametrize("dt,idx", PARAMS, ids=[f"{dt}-{R.case_id(CASES[i])}" for dt, i in PARAMS])
def test_conv_fwd_vs_fp64(ops, dt, idx):
    run_case(ops, dt, idx)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", RUN_TYPES)
def test_conv_fwd_reaches_every_kernel_and_form(ops, dt):
    """The routes the launches above reported (a row this session did not run is run here): every ConvKernel value with every ConvRoute::form its
    route function can produce was launched in this element type (named exception: no fp32 first-conv kernel).  Prints the FWDSUM lines."""
    for sub in ((dt, "bf16x2") if dt == "bf16" else (dt,)):
        for c in CASES:
            if sub in c["types"] and c["idx"] not in REACHED[sub]:
                run_case(ops, sub, c["idx"])
        by = {}
        for idx, kf in REACHED[sub].items():
            by.setdefault(kf, []).append(idx)
        wi = max(WORST[sub], key=WORST[sub].get)
        print(f"   FWDSUM conv fwd {sub}: worst err / budget {WORST[sub][wi]:.3f} ({CASES[wi]['name']}); kernels "
              + ", ".join(f"{KERNEL_NAMES[k]}/{f} x{len(v)}" for (k, f), v in sorted(by.items())))
        fam = {}
        for idx, (k, f) in REACHED[sub].items():
            fam[k] = max(fam.get(k, 0.0), WORST[sub][idx])
        print(f"   FWDFAM conv fwd {sub}: " + ", ".join(f"{KERNEL_NAMES[k]} {v:.3f}" for k, v in sorted(fam.items())))
        if sub in R.ALL3:
            assert set(by) == R.want_pairs(sub), f"{sub}: reached {sorted(by)}, wanted {sorted(R.want_pairs(sub))}"
        else:
            assert set(by) == {(R.K_IGEMM, 0)}
