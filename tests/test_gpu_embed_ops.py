"""GPU: the embedding path and the layout kernels, op by op, against plain fp64 torch on the CPU.

  timestep_embedding_kernel (csrc/embed.hip)         mi355_timestep_embedding   every dim x batch x max_period, four classes of |t|
  linear_small_kernel, linear_kernel                  mi355_linear               both kernels, the reported form asserted in every run
  label_emb_linear_kernel<16>, <8>                    mi355_label_emb_linear     both forms, three row-to-time mappings, labels out of range
  emb_gather_kernel                                   mi355_emb_gather           a bit-exact copy; labels out of range
  pack_nhwc_kernel, unpack_nchw_kernel                mi355_pack_nhwc, mi355_unpack_nchw          bit-exact in fp32, bf16, fp16
  unpack_channels_kernel (csrc/backward.hip)          mi355_unpack_channels      bit-exact; fp16 refused
  resample_kernel                                     mi355_resample             nearest x2 bit-exact; the 2x2 pool against fp64

References, input classes, case lists and budgets are those of tests/test_embed_ref_cpu.py, which proves on the CPU that the kernels' summation
order can meet the budgets and that twelve mutants cannot.  No case is skipped or filtered: every list is run whole.

Measured on the MI355X (worst error / budget per op; pack, unpack, gather and nearest x2 are bit-exact):
  timestep_embedding 0.30 | linear: small kernel 0.34, slab kernel 0.25 (B > 8) and 0.19 (B <= 8) | label_emb_linear 0.18
  resample 2x2 pool: fp32 0.61, bf16 1.00, fp16 1.00 of the tolerance (the store's half ulp is the whole of the 16-bit tolerance but 3 u32)
Before the slab kernels summed K in blocks of 32 (csrc/embed.hip linear_rows) a single fmaf chain gave 0.84 for the slab kernel at K = 2048
and failed label_emb_linear there: rows with labels out of range, R = 16, K = 2048, J = 129: 8.576e-07 against a budget of 8.434e-07.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mi355 import _lib
from mi355._lib import MI355BackendError
from mi355.synth import randn
from tests.test_embed_ref_cpu import (INT32_MIN, LABEL_CASES, LINEAR_CASES, bits, check_timestep, label_linear64, label_norm_err, label_runs,
                                      label_scale64, linear_budget, linear_runs, norm_err, pack_cases, pack_inputs, pack_ref, pool_tolerance,
                                      resample_cases, resample_input, timestep_cases, with_specials)

DEV = "cuda:0"
F32, BF16, BF16X2, F16 = _lib.MI355_F32, _lib.MI355_BF16, _lib.MI355_BF16X2, _lib.MI355_F16
ELEM = {F32: torch.float32, BF16: torch.bfloat16, BF16X2: torch.bfloat16, F16: torch.float16}
NAME = {F32: "fp32", BF16: "bf16", BF16X2: "bf16x2", F16: "fp16"}
SENTINEL = -12345.5


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def dev(t):
    return t.to(DEV) if t is not None else None


def refused(code, fn):
    """fn must raise the backend's error with that return code."""
    with pytest.raises(MI355BackendError, match=rf"\({code}\)"):
        fn()


# ---- timestep embedding ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_timestep_embedding_vs_fp64(ops):
    worst = 0.0
    for ci, t, dim, mp in timestep_cases():
        got = ops.timestep_embedding(dev(t), dim, mp).cpu()
        assert got.shape == (t.numel(), dim) and torch.isfinite(got).all()
        worst = max(worst, check_timestep(got, t, dim, mp, f"timestep dim={dim} B={t.numel()} max_period={mp:g}", report=print))
    print(f"   EMBSUM timestep_embedding: worst err / budget {worst:.3f}")


# ---- the linears ----------------------------------------------------------------------------------------------------------------------------
GROUPS = {"small": lambda B, K: B <= 8 and K % 32 == 0, "slab_big_batch": lambda B, K: B > 8, "slab_small_batch": lambda B, K: B <= 8 and K % 32 != 0}


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_linear_vs_fp64(ops, group):
    """All four activation settings, bias present and NULL, three input classes; the form asserted in every run; a guard row beyond B."""
    cases = [c for c in LINEAR_CASES if GROUPS[group](c[0], c[1])]
    assert cases and sum(len([c for c in LINEAR_CASES if g(c[0], c[1])]) for g in GROUPS.values()) == len(LINEAR_CASES)
    want_form = 1 if group == "small" else 0
    worst, on = 0.0, {}
    for tag, x, wt, b, ia, oa, form in linear_runs(LINEAR_CASES):
        B, K = x.shape
        if not GROUPS[group](B, K):
            continue
        for t in (x, wt, b):
            if t is not None and id(t) not in on:
                on[id(t)] = (t, dev(t))
        out = torch.full((B + 1, wt.shape[1]), SENTINEL, device=DEV)
        got, f = ops.linear(on[id(x)][1], on[id(wt)][1], on[id(b)][1] if b is not None else None, ia, oa, out=out)
        assert f == form == want_form, f"{tag}: form {f}, expected {want_form}"
        g = got.cpu()
        assert bool((g[B] == SENTINEL).all()), f"{tag}: the row beyond B was written"
        assert torch.isfinite(g[:B]).all(), f"{tag}: unwritten or non-finite outputs"
        e, bud = norm_err(g[:B], x, wt, b, ia, oa), linear_budget(K)
        worst = max(worst, e / bud)
        print(f"   EMBSTAT {tag} form {f}: err {e:.3e} budget {bud:.3e}")
        assert e <= bud, f"{tag}: normalised error {e:.3e} > budget {bud:.3e}"
    print(f"   EMBSUM linear {group}: worst err / budget {worst:.3f}")


@pytest.mark.gpu
def test_linear_refusals_launch_nothing(ops):
    for K in (2052, 6):
        x, wt = dev(randn(1, 9, K)), dev(randn(2, K, 16))
        out = torch.full((9, 16), SENTINEL, device=DEV)
        refused(-4, lambda: ops.linear(x, wt, None, out=out))
        torch.cuda.synchronize()
        assert bool((out.cpu() == SENTINEL).all()), f"K={K}: the refused call wrote the output"


# ---- the class-conditional linear -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_label_emb_linear_vs_fp64(ops):
    worst, forms = 0.0, set()
    for tag, d, R, ncls, form in label_runs(LABEL_CASES):
        K, J = d["wt"].shape
        g = {k: dev(v) if torch.is_tensor(v) else v for k, v in d.items()}
        out = torch.full((R + 1, J), SENTINEL, device=DEV)
        got, err, f = ops.label_emb_linear(g["h"], g["lemb"], g["wt"], g["bias"], R, d["h_div"], labels=g["labels"], out=out)
        forms.add(f)
        assert f == form, f"{tag}: form {f}, expected {form}"
        assert err == 0, f"{tag}: error word {err} with valid labels"
        valid = got.cpu()
        assert bool((valid[R] == SENTINEL).all()), f"{tag}: the row beyond R was written"
        assert torch.isfinite(valid[:R]).all(), f"{tag}: unwritten or non-finite outputs"
        e, bud = label_norm_err(valid[:R], d, R, ncls), linear_budget(K)
        worst = max(worst, e / bud)
        print(f"   EMBSTAT {tag} form {f}: err {e:.3e} budget {bud:.3e}")
        assert e <= bud, f"{tag}: normalised error {e:.3e} > budget {bud:.3e}"
        if d["labels"] is None:
            continue
        # labels out of range: -1, n_classes, INT32_MIN at the first, a middle and the last row
        bad_rows = sorted({0, R // 2, R - 1})
        labels = d["labels"].clone()
        for i, r in enumerate(bad_rows):
            labels[r] = (-1, ncls, INT32_MIN)[(i + R) % 3]
        out = torch.full((R + 1, J), SENTINEL, device=DEV)
        got, err, f = ops.label_emb_linear(g["h"], g["lemb"], g["wt"], g["bias"], R, d["h_div"], labels=dev(labels), out=out)
        assert err == 2 and f == form, f"{tag}: bad labels: error word {err}, form {f}"
        bad = got.cpu()
        keep = torch.ones(R + 1, dtype=torch.bool)
        keep[bad_rows] = False
        assert torch.equal(bits(bad[keep]), bits(valid[keep])), f"{tag}: a bad label changed another row"
        args = (d["h"], d["h_div"], d["lemb"], labels, ncls, d["wt"], d["bias"], R)   # the reference gives a bad label no label term: silu(h) Wt + b
        eb = float(((bad[:R].double() - label_linear64(*args)).abs() / label_scale64(*args))[bad_rows].max())
        worst = max(worst, eb / bud)
        assert eb <= bud, f"{tag}: rows with bad labels off by {eb:.3e} > budget {bud:.3e}"
    print(f"   EMBSUM label_emb_linear forms {sorted(forms)}: worst err / budget {worst:.3f}")
    assert forms == {8, 16}
    h, lemb, wt = dev(randn(3, 2, 2052)), dev(randn(4, 3, 2052)), dev(randn(5, 2052, 8))
    out = torch.full((2, 8), SENTINEL, device=DEV)
    refused(-4, lambda: ops.label_emb_linear(h, lemb, wt, None, 2, 1, labels=dev(torch.zeros(2, dtype=torch.int32)), out=out))
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENTINEL).all())


@pytest.mark.gpu
def test_emb_gather_is_a_bit_exact_copy(ops):
    ncls = 7
    for ci, (B, J) in enumerate([(B, J) for B in (1, 3, 65) for J in (4, 12, 260, 1000)]):
        table = with_specials(randn(600 + ci, ncls, J), ci)
        labels = torch.from_numpy(np.random.RandomState(610 + ci).randint(0, ncls, size=B).astype(np.int32))
        out = torch.full((B + 1, J), SENTINEL, device=DEV)
        got, err = ops.emb_gather(dev(table), dev(labels), out=out)
        got = got.cpu()
        tag = f"gather B={B} J={J}"
        assert err == 0, f"{tag}: error word {err} with valid labels"
        assert torch.equal(bits(got[:B]), bits(table[labels.long()])) and bool((got[B] == SENTINEL).all()), tag
        bad_rows = sorted({0, B // 2, B - 1})
        bad = labels.clone()
        for i, r in enumerate(bad_rows):
            bad[r] = (-1, ncls, INT32_MIN)[(i + ci) % 3]
        want = table[bad.long().clamp(0, ncls - 1)].clone()
        want[bad_rows] = 0.0
        out = torch.full((B + 1, J), SENTINEL, device=DEV)
        got, err = ops.emb_gather(dev(table), dev(bad), out=out)
        got = got.cpu()
        assert err == 2, f"{tag}: bad labels: error word {err}"
        assert torch.equal(bits(got[:B]), bits(want)) and bool((got[B] == SENTINEL).all()), f"{tag}: bad labels"
    out = torch.full((2, 6), SENTINEL, device=DEV)
    refused(-2, lambda: ops.emb_gather(dev(randn(1, ncls, 6)), dev(torch.zeros(2, dtype=torch.int32)), out=out))
    torch.cuda.synchronize()
    assert bool((out.cpu() == SENTINEL).all())


# ---- pack / unpack --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16, BF16X2], ids=["fp32", "bf16", "fp16", "bf16x2"])
def test_pack_nhwc_is_torchs_round_to_nearest_even_cast(ops, dtype):
    for ci, B, hw, cx, cc, cpad in pack_cases(ELEM[dtype]):
        x, cond = pack_inputs(ci, B, hw, cx, cc)
        got = ops.pack_nhwc(dev(x), dev(cond), cpad=cpad, dtype=dtype).cpu()
        want = pack_ref(x, cond, cpad, ELEM[dtype])
        diff = bits(got) != bits(want)
        assert not bool(diff.any()), (f"{NAME[dtype]} pack B={B} HW={hw} C={cx}+{cc} -> {cpad}: {int(diff.sum())} elements differ from torch's cast, first: "
                                      f"got {got[diff][:4].tolist()} want {want[diff][:4].tolist()}")
    if dtype != F32:
        refused(-2, lambda: ops.pack_nhwc(dev(randn(1, 1, 3, 4)), cpad=4, dtype=dtype))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_unpack_nchw_is_an_exact_widening_transpose(ops, dtype):
    for ci, B, hw, cx, cc, cpad in pack_cases(ELEM[dtype]):
        x, cond = pack_inputs(ci, B, hw, cx, cc)
        t = pack_ref(x, cond, cpad, ELEM[dtype])          # values of the element type, inf and subnormals among them
        got = ops.unpack_nchw(dev(t), dtype=dtype).cpu()
        assert torch.equal(bits(got), bits(t.float().permute(0, 2, 1).contiguous())), f"{NAME[dtype]} unpack B={B} HW={hw} C={cpad}"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, BF16X2], ids=["fp32", "bf16", "bf16x2"])
def test_unpack_channels_is_an_exact_slice(ops, dtype):
    ci = 0
    for stride in (8, 32):
        for c0 in (0, 3):
            for count in (1, 3):
                for B, hw in ((1, 49), (3, 35)):
                    ci += 1
                    assert c0 + count < stride
                    t = with_specials(randn(700 + ci, B, hw, stride), ci).to(ELEM[dtype])
                    got = ops.unpack_channels(dev(t), c0, count, dtype=dtype).cpu()
                    want = t[:, :, c0:c0 + count].float().permute(0, 2, 1).contiguous()
                    assert torch.equal(bits(got), bits(want)), f"{NAME[dtype]} unpack_channels B={B} HW={hw} stride={stride} c0={c0} count={count}"


@pytest.mark.gpu
def test_unpack_channels_refuses_fp16(ops):
    t = dev(torch.zeros(1, 4, 8, dtype=torch.float16))
    refused(-4, lambda: ops.unpack_channels(t, 0, 1, dtype=F16))


# ---- resample ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
def test_resample_vs_interpolate_and_fp64_pool(ops, dtype):
    td = ELEM[dtype]
    worst = 0.0
    for ci, N, C, Hs, Ws in resample_cases():
        x = resample_input(ci, N, C, Hs, Ws, td)                       # NCHW fp32 holding values of the type
        t = dev(x.permute(0, 2, 3, 1).contiguous().to(td))
        tag = f"{NAME[dtype]} resample N={N} C={C} {Hs}x{Ws}"
        up = ops.resample(t, "up", dtype=dtype).cpu()
        want = F.interpolate(x, scale_factor=2, mode="nearest").permute(0, 2, 3, 1).contiguous().to(td)
        assert torch.equal(bits(up), bits(want)), f"{tag}: nearest x2"
        pool = ops.resample(t, "pool", dtype=dtype).cpu()
        assert pool.shape == (N, Hs // 2, Ws // 2, C) and torch.isfinite(pool.float()).all(), f"{tag}: pool shape or unwritten outputs"
        ref = F.avg_pool2d(x.double(), 2)
        err = (pool.double().permute(0, 3, 1, 2) - ref).abs()
        tol = pool_tolerance(x.double(), ref, td)
        worst = max(worst, float((err / tol).max()))
        assert float((err - tol).max()) <= 0, f"{tag}: pool off by {float((err - tol).max()):.3e} beyond its tolerance"
    print(f"   EMBSUM resample pool {NAME[dtype]}: worst err / tolerance {worst:.3f}")


# ---- the wrappers' own checks (no GPU needed) -------------------------------------------------------------------------------------------------
def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    from mi355.ops import default_ops as ops

    x, wt = torch.zeros(2, 32), torch.zeros(32, 8)
    with pytest.raises(MI355BackendError, match="device tensors"):
        ops.linear(x, wt)
    with pytest.raises(MI355BackendError, match="device tensors"):
        ops.label_emb_linear(x, torch.zeros(3, 32), wt, None, 2, 1, labels=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(MI355BackendError, match="device tensors"):
        ops.emb_gather(torch.zeros(3, 8), torch.zeros(2, dtype=torch.int32))
    with pytest.raises(MI355BackendError, match="device tensors"):
        ops.pack_nhwc(torch.zeros(1, 3, 4), dtype=BF16)
    for fn in (lambda t: ops.unpack_nchw(t, dtype=BF16), lambda t: ops.unpack_channels(t, 0, 1, dtype=BF16), lambda t: ops.resample(t[None], "up", dtype=BF16)):
        with pytest.raises(MI355BackendError, match="device tensors"):
            fn(torch.zeros(1, 4, 8, dtype=torch.bfloat16))
    if torch.cuda.is_available():
        with pytest.raises(TypeError):
            ops.linear(dev(x.double()), dev(wt))
        with pytest.raises(TypeError):
            ops.emb_gather(dev(torch.zeros(3, 8)), dev(torch.zeros(2, dtype=torch.int64)))
        with pytest.raises(TypeError):
            ops.unpack_nchw(dev(torch.zeros(1, 4, 8)), dtype=BF16)
    with pytest.raises(ValueError):
        ops.linear(x, torch.zeros(16, 8))
    with pytest.raises(ValueError):
        ops.unpack_channels(torch.zeros(1, 4, 8), 6, 3)
