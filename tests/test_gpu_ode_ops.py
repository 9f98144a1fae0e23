"""GPU: the three kernels of csrc/ode.hip (rk_combine, rk_sqnorm, rk_interp) op by op against fp64 evaluations of the same expressions,
at ragged sizes and misaligned views, then one Dormand-Prince step and whole adaptive solves on them against the analytic solution and
the CPU stand-in solve of tests/test_dopri5_cpu.py."""
import pytest
import torch

from mi355.ode import Dopri5
from mi355.synth import randn
from tests.test_dopri5_cpu import ROWS, N, TIMES, CpuOps, _exact, _problem, solve_cpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24      # unit roundoff of fp32 (round to nearest)
SENTINEL = -777.25


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def _view(t, off, pad=8):
    """A contiguous device copy of 1-D `t` whose storage starts `off` elements into an allocation (off % 4 != 0: not 16-byte aligned)."""
    base = torch.full((t.numel() + pad,), SENTINEL, device=DEV, dtype=t.dtype)
    v = base[off: off + t.numel()]
    v.copy_(t)
    assert v.is_contiguous() and v.storage_offset() == off
    return base, v


COEFFS = [0.37, -1.25e-3, 0.0, 7.5, -0.04, 3.0e-6, -2.0]     # mixed sign and magnitude, one zero
SIZES = [1, 3, 4, 5, 1023, 1024, 1025, 3 * 32 * 32 * 64 + 2]


def _combine_case(ops, n, nk, with_y0, offs=(0, 0, 0), seed=0):
    """offs: storage offsets of (out, y0, the last k).  Checks the bound and the guard region around `out`."""
    ks = [randn(100 * seed + j + 1, n) for j in range(nk)]
    y0 = randn(100 * seed + 50, n) * 3.0 if with_y0 else None
    c32 = torch.tensor(COEFFS[:nk], dtype=torch.float32)
    ref = torch.zeros(n, dtype=torch.float64) if y0 is None else y0.double().clone()
    mag = torch.zeros(n, dtype=torch.float64) if y0 is None else y0.double().abs()
    for j in range(nk):
        term = c32[j].double() * ks[j].double()
        ref += term
        mag += term.abs()
    base, out = _view(torch.full((n,), SENTINEL), offs[0], pad=64)
    dks = [k.to(DEV) for k in ks]
    if nk:
        dks[-1] = _view(ks[-1], offs[2])[1]
    dy0 = _view(y0, offs[1])[1] if with_y0 else None
    ops.rk_combine(out, dy0, dks, COEFFS[:nk])
    got = base.cpu()
    o = offs[0]
    assert (got[:o] == SENTINEL).all() and (got[o + n:] == SENTINEL).all(), "rk_combine wrote outside its output"
    err = (got[o: o + n].double() - ref).abs()
    # every product and every add rounds at most once (an fma rounds less): nk products, nk adds, one margin; a zero bound means exact
    bound = (nk + 2) * U * mag
    worst = (err / bound.clamp_min(1e-300)).max().item() if n else 0.0
    assert (err <= bound).all(), (n, nk, with_y0, offs, worst)
    return worst


@pytest.mark.parametrize("with_y0", [True, False])
@pytest.mark.parametrize("nk", [0, 1, 3, 7])
def test_rk_combine(ops, nk, with_y0):
    worst = max(_combine_case(ops, n, nk, with_y0, seed=i) for i, n in enumerate(SIZES))
    print(f"rk_combine nk={nk} y0={with_y0}: worst |err| / bound = {worst:.3f}")
    # measured on an MI355X, worst |err| / bound (with y0, without): nk 0: 0, 0;  nk 1: 0.54, 0.33;  nk 3: 0.43, 0.39;  nk 7: 0.41, 0.37


def test_rk_combine_empty_is_a_no_op(ops):
    e = torch.empty(0, device=DEV)
    assert ops.rk_combine(e, e, [e, e], [0.5, 0.25]).numel() == 0
    acc = torch.full((1,), 2.5, device=DEV, dtype=torch.float64)
    ops.rk_sqnorm(acc, e, e, e, e, 1e-3, 1e-2)
    assert acc.item() == 2.5
    assert ops.rk_interp(e, e, e, e, e, e, 0.1, 0.5).numel() == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("off", [1, 2, 3])
def test_rk_combine_misaligned_views(ops, off):
    """A contiguous view whose storage offset is not a multiple of 4 elements is not 16-byte aligned: the kernel must take its scalar
    path when ANY of its pointers is such a view (out, y0 or a stage), and give the same answer to the same bound."""
    for n in (5, 1025, 4099):
        for offs in ((off, 0, 0), (0, off, 0), (0, 0, off), (off, (off + 1) % 4, (off + 2) % 4)):
            _combine_case(ops, n, 3, True, offs=offs, seed=7)
        _combine_case(ops, n, 7, False, offs=(off, 0, off), seed=8)


def _sqnorm_ref(a, sub, b, b2, atol, rtol):
    """fp64 sum of squares of the fp32-evaluated ratios (eager fp32 torch on the CPU)."""
    num = a if sub is None else a - sub
    mag = torch.zeros_like(a) if b is None else b.abs()
    if b2 is not None:
        mag = torch.maximum(mag, b2.abs())
    r = num / (torch.tensor(atol, dtype=torch.float32) + torch.tensor(rtol, dtype=torch.float32) * mag)
    return (r.double() ** 2).sum().item()


# Dopri5 calls: _norm(y0, b=y0), _norm(f1, sub=f0, b=y0), _norm(err, b=y0, b2=y1); and the bare rms norm (atol 1, rtol 0)
SQNORM_ARGS = {"plain": (False, False, False), "b": (False, True, False), "sub_b": (True, True, False), "b_b2": (False, True, True)}


@pytest.mark.parametrize("combo", sorted(SQNORM_ARGS))
def test_rk_sqnorm(ops, combo):
    use_sub, use_b, use_b2 = SQNORM_ARGS[combo]
    atol, rtol = (1.0, 0.0) if combo == "plain" else (1e-3, 1e-2)     # atol > 0: no denominator near zero
    worst = 0.0
    for i, n in enumerate((1, 63, 256, 257, 4099, 2048 * 256 + 1000, 3 * 2048 * 256 + 5)):     # the last two: > 1 trip of the grid-stride loop
        a, sub, b, b2 = (randn(10 * i + j + 1, n) * s for j, s in enumerate((1.0, 1.0, 2.0, 3.0)))
        sub, b, b2 = (sub if use_sub else None), (b if use_b else None), (b2 if use_b2 else None)
        want = _sqnorm_ref(a, sub, b, b2, atol, rtol)
        dev = [None if t is None else t.to(DEV) for t in (a, sub, b, b2)]
        acc = torch.zeros(1, device=DEV, dtype=torch.float64)
        ops.rk_sqnorm(acc, *dev, atol, rtol)
        # into a non-zero slot of a longer vector: the neighbours stay, the slot gains the same sum
        vec = torch.tensor([1.5, 100.0, -3.0], device=DEV, dtype=torch.float64)
        ops.rk_sqnorm(vec[1:2], *dev, atol, rtol)
        got, vec = acc.item(), vec.tolist()
        rel = abs(got - want) / want
        worst = max(worst, rel)
        # all terms positive (no cancellation); per term a few roundings of 2^-24 (the fma in the denominator, the division, the
        # difference), doubled by the square: 1e-6 = 16.8 * 2^-24
        assert rel <= 1e-6, (combo, n, got, want)
        assert vec[0] == 1.5 and vec[2] == -3.0 and abs(vec[1] - 100.0 - want) <= 1e-6 * want + 1e-12, (combo, n, vec, want)
    print(f"rk_sqnorm {combo}: worst relative difference {worst:.2e}")
    # measured on an MI355X: plain 1.2e-15, b 4.7e-08, sub_b 4.5e-08, b_b2 7.0e-08


def test_rk_sqnorm_b2_is_a_maximum(ops):
    """max(|b|, |b2|), whichever is larger, element by element: the scale of the accept/reject ratio."""
    n = 1000
    a, b = randn(1, n), randn(2, n)
    big = b * 50.0
    lo = torch.zeros(1, device=DEV, dtype=torch.float64)
    hi = torch.zeros(1, device=DEV, dtype=torch.float64)
    ops.rk_sqnorm(lo, a.to(DEV), None, b.to(DEV), big.to(DEV), 1e-3, 1.0)
    ops.rk_sqnorm(hi, a.to(DEV), None, big.to(DEV), b.to(DEV), 1e-3, 1.0)
    want = _sqnorm_ref(a, None, big, None, 1e-3, 1.0)
    assert abs(lo.item() - want) <= 1e-6 * want and abs(hi.item() - want) <= 1e-6 * want


@pytest.mark.parametrize("x", [0.0, 0.25, 0.5, 1.0])
def test_rk_interp(ops, x):
    dt = 0.137
    worst = 0.0
    for i, n in enumerate((1, 3, 255, 257, 1023, 4099)):
        y0, y1, ym, f0, f1 = (randn(20 * i + j + 1, n) * s for j, s in enumerate((1.0, 1.2, 1.1, 4.0, 3.0)))
        d = [t.double() for t in (y0, y1, ym, f0, f1)]
        Y0, Y1, YM, F0, F1 = d
        h = torch.tensor(dt, dtype=torch.float32).double()
        xx = torch.tensor(x, dtype=torch.float32).double()
        a = 2 * h * (F1 - F0) - 8 * (Y1 + Y0) + 16 * YM
        b = h * (5 * F0 - 3 * F1) + 18 * Y0 + 14 * Y1 - 32 * YM
        c = h * (F1 - 4 * F0) - 11 * Y0 - 5 * Y1 + 16 * YM
        ref = (((a * xx + b) * xx + c) * xx + h * F0) * xx + Y0
        A0, A1, AM, G0, G1 = (t.abs() for t in d)
        mag = (xx ** 4 * (2 * h * (G1 + G0) + 8 * (A1 + A0) + 16 * AM) + xx ** 3 * (h * (5 * G0 + 3 * G1) + 18 * A0 + 14 * A1 + 32 * AM)
               + xx ** 2 * (h * (G1 + 4 * G0) + 11 * A0 + 5 * A1 + 16 * AM) + xx * h * G0 + A0)
        out = torch.full((n + 16,), SENTINEL, device=DEV)
        ops.rk_interp(out[:n], *(t.to(DEV) for t in (y0, y1, ym, f0, f1)), dt, x)
        got = out.cpu()
        assert (got[n:] == SENTINEL).all()
        err = (got[:n].double() - ref).abs()
        # roundings on the longest path, every operation rounded once (an fma only removes some): inside b, 5 f0 (1), - 3 f1 (2), * dt (3),
        # + 18 y0 (4), + 14 y1 (5), - 32 ym (6); then + b (7), * x (8), + c (9), * x (10), + d (11), * x (12), + e (13).  The path
        # through a is one shorter (4 inside a, * x, then the same tail).  Each rounding is relative to a partial sum that the sum of
        # absolute terms bounds.
        bound = 13 * U * mag
        assert (err <= bound).all(), (x, n, (err / bound).max().item())
        worst = max(worst, (err / bound).max().item())
        if x == 0.0:
            assert torch.equal(got[:n], y0)
    print(f"rk_interp x={x}: worst |err| / bound = {worst:.3f}")
    # measured on an MI355X, worst |err| / bound: x = 0: 0 (exact);  0.25: 0.094;  0.5: 0.089;  1: 0.095


# ---- the solver on the HIP ops -----------------------------------------------------------------------------------------------------------

def _gpu_problem():
    S, y0, _ = _problem()
    St = S.T.contiguous().float().to(DEV)
    return S, y0, (lambda t, y: [y[0] @ St])


def test_one_step_on_the_hip_ops():
    """One step of size 0.4 (error estimate 6e-3, far above rounding) against the same step in fp64 on the CPU stand-in.
    Worst-case rounding budget, from the data: a stage y0 + h sum(beta_j k_j) has at most 7 terms, so (7 + 2) roundings of 2^-24 relative
    to |y| + h * sum|beta| * |f| with sum|beta| <= 25 (row 4 of BETA); 8 combinations (6 stages, error estimate, midpoint), doubled for
    what earlier stages pass on through f (h * |beta| * Lipschitz constant 3 < 2 per stage, damped by the small weights that follow).
    A wrong weight moves the result by a stage term h * |f| ~ 1.  The dense output adds its own 13 roundings relative to the sum of its
    absolute terms (<= 66 |y| + 10 h |f|) and passes node differences on with Hermite weights < 1.5 each."""
    h = 0.4
    S, y0, f = _gpu_problem()
    y32 = y0.float()
    _, _, f64 = _problem()
    ref = Dopri5(f64, 1e-6, 1e-6, ops=CpuOps(), dtype=torch.float64)
    r0 = [y32.double()]
    rf0 = ref._f(0.0, r0)
    ry1, rf1, rerr, rks = ref._step(0.0, h, r0, rf0)
    rmid = ref._midpoint(r0, rks, h)
    sol = Dopri5(f, 1e-6, 1e-6)
    g0 = [y32.to(DEV)]
    gf0 = sol._f(0.0, g0)
    gy1, gf1, gerr, gks = sol._step(0.0, h, g0, gf0)
    gmid = sol._midpoint(g0, gks, h)
    assert sol.nfe == 7 and gy1[0].dtype == torch.float32
    ymax = max(t.abs().max().item() for t in (r0[0], ry1[0], rmid[0]))
    fmax = max(k[0].abs().max().item() for k in rks)
    node_bound = 2 * 8 * 9 * U * (ymax + h * 25 * fmax)
    dense_bound = 13 * U * (66 * ymax + 10 * h * fmax) + 3 * 1.5 * node_bound
    nodes = {"y1": (gy1[0].cpu().double() - ry1[0]).abs().max().item(), "err": (gerr[0].cpu().double() - rerr[0]).abs().max().item(),
             "ymid": (gmid[0].cpu().double() - rmid[0]).abs().max().item()}
    dense = {}
    for x in (0.25, 0.8):
        gd = sol._dense((g0, gy1, gmid, gf0, gf1, 0.0, h), x * h)[0].cpu().double()
        rd = ref._dense((r0, ry1, rmid, rf0, rf1, 0.0, h), x * h)[0]
        dense[x] = (gd - rd).abs().max().item()
    print(f"one step h={h} on HIP vs fp64: nodes {nodes} (bound {node_bound:.2e}), dense {dense} (bound {dense_bound:.2e}); "
          f"|err estimate| = {rerr[0].abs().max().item():.2e}, max|y| {ymax:.2f}, max|f| {fmax:.2f}")
    # measured on an MI355X: y1 1.2e-6, err 1.4e-7, ymid 2.9e-7 (bound 6.1e-4); dense 5.3e-7 (x = 0.25), 3.8e-6 (0.8) (bound 3.0e-3);
    # |err estimate| 6.2e-3, max|y| 3.66, max|f| 6.79
    assert max(nodes.values()) <= node_bound, (nodes, node_bound)
    assert max(dense.values()) <= dense_bound, (dense, dense_bound)
    assert rerr[0].abs().max().item() >= 10 * node_bound     # the step is large enough for the comparison to mean something


@pytest.mark.parametrize("tol", [1e-3, 1e-4, 1e-5, 1e-6])
def test_adaptive_solve_on_the_hip_ops(tol):
    S, y0, f = _gpu_problem()
    sol = Dopri5(f, tol, tol)
    outs = [o[0].cpu() for o in sol.integrate_times([y0.float().to(DEV)], TIMES)]
    y0r = y0.float().double()
    ratios = [(o.double() - _exact(S, y0r, t)).abs().max().item() / tol for o, t in zip(outs, TIMES[1:])]
    cpu, cpu_outs = solve_cpu(tol)
    d = (outs[-1] - cpu_outs[-1]).abs().max().item() / tol
    print(f"adaptive on HIP, tol {tol:g}: max|err| / tol at t = {TIMES[1:]}: {ratios}; vs CPU stand-in {d:.3f} tol; nfe {sol.nfe} (CPU {cpu.nfe})")
    # measured on an MI355X (err / tol at 0.25, 0.6, 1.0; difference to the CPU stand-in in tol; nfe HIP / CPU):
    # 1e-3: 3.7, 6.1, 8.5; 0.005; 26 / 26.   1e-4: 1.4, 5.5, 7.3; 0.007; 38 / 38.   1e-5: 2.7, 4.7, 6.8; 0.20; 50 / 50.
    # 1e-6: 2.3, 4.0, 6.0; 6.4; 74 / 74 (at 1e-6 the tolerance is 17 ulp of the state: both solves are rounding-limited).
    assert max(ratios) <= 20.0
    assert d <= 10.0                # same steps, different rounding; a flipped accept/reject moves the result by < the tolerance
    assert abs(sol.nfe - cpu.nfe) <= 6 and sol.nfe == 6 * sol.n_steps + 2
    assert outs[0].shape == (ROWS, N)
