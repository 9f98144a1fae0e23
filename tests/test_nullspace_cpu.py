"""CPU: the null-space (DDNM) samplers - the operator algebra of the fp64 restatement (tests/nullspace_ref.py), DDPM.nullspace_coefs, the element-wise
budget of mi355_nullspace_step proven on an fp32 restatement in the kernel's operation order, the Python surface (NullSpace, AveragePooling, the
refusals, the walk), the generic host loop on CPU tensors, and the library's refusals that need no device.

Budget of the step (the form of tests/test_ddpm_respace_cpu.py: every fp32 rounding is at most 2^-24 of the magnitude of its result, a magnitude is
bounded by the sum of the magnitudes that enter it; against fp64 from the same fp32 inputs).  With E = 2^-24:
  x0   : e_x0 = r_pre E P,  r_pre = 3 (eps: P = |a x| + |b o|; v: P = |sa x| + |sb o|), 0 (x0: the output itself); the clip is exact and 1-Lipschitz
  A(x0): the n_taps - 1 sums of a row in the worst order, each on at most the row's weighted magnitude A(|x0|), one more rounding for kind 1's
         division, and the inputs' own errors: e_A = (n_taps - 1 + div) E A(|x0|) + A(e_x0)
  r    : e_r = e_A + E (|A(x0)| + |y|);   t = lam r: e_t = lam e_r + E |t|
  x0h  : e_h = e_x0 + e_t + E (|x0| + |t|) on a tap, e_x0 elsewhere
  form 0: e = c1 e_h + E (2 |c1 x0h| + 2 |c2 x| + |sigma z| + (|c1 x0h| + |c2 x| + |sigma z|))
  form 1: a x: E |a x|;  num = a x - x0h: e_n = E |a x| + e_h + E (|a x| + |x0h|);  e2 = num / b: e_e2 = e_n / b + E (|a x| + |x0h|) / b;
          the host coefficients: d_sa = E sa;  d_sb = d(sb^2) / (2 sb) + E sb with d(sb^2) = E ((1 - p) + s^2 + |1 - p - s^2|) (sqrt(d(sb^2)) where sb = 0);
          m: e = sa e_h + |x0h| d_sa + sb e_e2 + |e2| d_sb + E (2 sa |x0h| + 2 sb |e2|);  with noise + E (2 |sigma z| + |m|)
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import nullspace_ref as NR

EPS32 = 2.0 ** -24
STEPS7 = [0, 3, 4, 17, 40, 41, 99]
STOL = dict(rtol=2e-3, atol=1e-3)
PREDS = ("eps", "x0", "v")
R_PRE = {"eps": 3, "x0": 0, "v": 3}
# (B, C, H, W, h_low, w_low): odd factor with W % 4 != 0; even anisotropic; one group per plane; factor 1; sy = 32
BAND_SHAPES = [(2, 1, 6, 9, 2, 3), (3, 2, 8, 12, 4, 3), (1, 3, 16, 16, 1, 1), (2, 3, 5, 7, 5, 7), (2, 1, 64, 20, 2, 5)]
MASK_SHAPES = [(3, 1, 5, 7), (3, 1, 16, 16)]      # n = 105 and 768


def _chain():
    from image_diffusion.sde_diffusion import DDPM

    return DDPM(100).respace(STEPS7)


def make_op(kind, shape, seed=0):
    """-> (operator dict of the restatement, the shape of its measurement)."""
    if kind == 0:
        known = np.random.default_rng(seed).random(shape[:4]) < 0.6
        return dict(kind=0, known=known), tuple(shape[:4])
    B, Cc, H, W, hl, wl = shape
    return dict(kind=kind, hl=hl, wl=wl), (B, Cc, hl, wl)


def step_cases():
    """Per-step scalars at three steps of a respaced chain, two lam each: (form 0 with the posterior's sigma, form 1 with DDIM(0.5)'s)."""
    r = _chain()
    T = r.host_tables()
    sg = r.ddim_sigma(0.5)
    out = []
    for k in (0, 3, r.Ns - 1):
        for lam in (1.0, 0.37):
            base = dict(cr=float(T["sqrt_recip_alphas_cumprod"][k]), crm1=float(T["sqrt_recipm1_alphas_cumprod"][k]),
                        sa=float(T["sqrt_alphas_cumprod"][k]), sb=float(T["sqrt_one_minus_alphas_cumprod"][k]), lam=lam)
            f0 = dict(base, a=float(T["posterior_mean_coef1"][k]), b=float(T["posterior_mean_coef2"][k]),
                      sigma=float(np.exp(np.float32(0.5) * T["posterior_log_variance_clipped"][k].numpy())))
            f1 = dict(base, a=float(T["alphas_cumprod_prev"][k]), b=0.0, sigma=float(sg[k]))
            out.append((k, f0, f1))
    return out


def ns_operands(kind, shape, pred, c, seed, nan=True):
    """x, out, y, z (fp32) and the operator: about a third of x0_pre outside [-1, 1], one planted NaN in x (in out for the x0 kind, which does not read
    x for its prediction), the measurement that of an unrelated image (kind 0: pad -2 at the unknown pixels)."""
    rng = np.random.default_rng(seed)
    op, yshape = make_op(kind, shape, seed + 1)
    xs = tuple(shape[:4])
    f = np.float32
    pre = rng.uniform(-1.5, 1.5, xs)
    if pred == "x0":
        out = pre.astype(f)
        x = rng.standard_normal(xs).astype(f)
    elif pred == "v":
        x = rng.standard_normal(xs).astype(f)
        out = ((float(f(c["sa"])) * x.astype(np.float64) - pre) / float(f(c["sb"]))).astype(f)
    else:
        out = rng.standard_normal(xs).astype(f)
        x = ((pre + float(f(c["crm1"])) * out.astype(np.float64)) / float(f(c["cr"]))).astype(f)
    z = rng.standard_normal(xs).astype(f)
    truth = rng.uniform(-1, 1, xs)
    y = NR.apply_A(op, truth).astype(f)
    if kind == 0:
        y = np.where(op["known"], y, f(-2.0)).astype(f)
    if nan:
        flat = (out if pred == "x0" else x).reshape(-1)
        flat[flat.size // 5] = np.nan
    assert y.shape == yshape
    return x, out, y, z, op


def ns_budget(op, pred, form, x, out, y, z, c):
    """-> (the fp64 step from the fp32 inputs, its element-wise budget as derived in the module docstring)."""
    E = EPS32
    c = {k: float(np.float32(v)) for k, v in c.items()}
    x64, o64, y64 = x.astype(np.float64), out.astype(np.float64), y.astype(np.float64)
    z64 = None if z is None else z.astype(np.float64)
    with np.errstate(invalid="ignore"):
        want, d = NR.step(op, pred, form, x64, o64, y64, z64, c, detail=True)
        P = {"eps": np.abs(c["cr"] * x64) + np.abs(c["crm1"] * o64), "x0": np.abs(o64), "v": np.abs(c["sa"] * x64) + np.abs(c["sb"] * o64)}[pred]
        e_x0 = R_PRE[pred] * E * P
        shape = x.shape
        nt = NR.n_taps(op, shape[2], shape[3])
        div = 1 if op["kind"] == 1 else 0
        e_A = (nt - 1 + div) * E * NR.apply_A(op, np.abs(d["x0"])) + NR.apply_A(op, e_x0)
        e_r = e_A + E * (np.abs(d["Ax"]) + np.abs(y64))
        e_t = c["lam"] * e_r + E * np.abs(d["t"])
        taps = NR.tap_mask(op, shape)
        e_h = np.where(taps, e_x0 + NR.spread(op, e_t, shape) + E * (np.abs(d["x0"]) + NR.spread(op, np.abs(d["t"]), shape)), e_x0)
        x0h = d["x0h"]
        sz = 0.0 if z64 is None else np.abs(c["sigma"] * z64)
        if form == 0:
            m1, m2 = np.abs(c["a"] * x0h), np.abs(c["b"] * x64)
            bound = abs(c["a"]) * e_h + E * (2 * m1 + 2 * m2 + sz + (m1 + m2 + sz))
        else:
            p, s, b = c["a"], c["sigma"], c["crm1"]
            sa, sb = NR.ddim_coefs(p, s)
            ax = np.abs(c["cr"] * x64)
            e_n = E * ax + e_h + E * (ax + np.abs(x0h))
            e_e2 = e_n / b + E * (ax + np.abs(x0h)) / b
            e2 = np.abs((c["cr"] * x64 - x0h) / b)
            d_sb2 = E * ((1.0 - p) + s * s + abs(1.0 - p - s * s))
            d_sb = d_sb2 / (2 * sb) + E * sb if sb > 0 else math.sqrt(d_sb2)
            bound = sa * e_h + np.abs(x0h) * E * sa + sb * e_e2 + e2 * d_sb + E * (2 * sa * np.abs(x0h) + 2 * sb * e2)
            if z64 is not None:
                bound = bound + E * (2 * sz + np.abs(want))
    return want, bound


def _ratio(got, want, bound):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), "the NaN pattern is not the reference's"
    return float((np.abs(got.astype(np.float64) - want)[~nan] / np.maximum(bound[~nan], 1e-300)).max()), nan


# ---- the operators ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape", [(0, s) for s in MASK_SHAPES] + [(k, s) for k in (1, 2) for s in BAND_SHAPES])
def test_operator_algebra(kind, shape):
    rng = np.random.default_rng(11)
    op, yshape = make_op(kind, shape, 5)
    xs = tuple(shape[:4])
    x0 = rng.uniform(-1, 1, xs)
    y = rng.uniform(-1, 1, yshape)
    rows = op["known"] if kind == 0 else np.ones(yshape, dtype=bool)
    # A A^+ = I on the rows
    assert np.abs(NR.apply_A(op, NR.pinv(op, y, xs)) - y)[rows].max() <= 1e-15
    # lam = 1: A(x0h) = y
    x0h = x0 - NR.pinv(op, np.where(rows, NR.apply_A(op, x0) - y, 0.0), xs)
    assert np.abs(NR.apply_A(op, x0h) - y)[rows].max() <= 4e-16 * NR.n_taps(op, xs[2], xs[3])
    # the null-space content is kept: (I - A^+ A) x0h = (I - A^+ A) x0
    null = lambda v: v - NR.pinv(op, np.where(rows, NR.apply_A(op, v), 0.0), xs)   # noqa: E731
    assert np.abs(null(x0h) - null(x0)).max() <= 1e-15
    # idempotence: rectifying the rectified prediction changes nothing
    again = x0h - NR.pinv(op, np.where(rows, NR.apply_A(op, x0h) - y, 0.0), xs)
    assert np.abs(again - x0h).max() <= 1e-15
    # pixels outside the taps pass through untouched
    assert np.array_equal(x0h[~NR.tap_mask(op, xs)], x0[~NR.tap_mask(op, xs)])
    t = torch.from_numpy(x0)
    if kind == 1:
        sy, sx = xs[2] // op["hl"], xs[3] // op["wl"]
        assert np.abs(NR.apply_A(op, x0) - F.avg_pool2d(t, (sy, sx), (sy, sx)).numpy()).max() <= 1e-15
    if kind == 2:
        ref = F.interpolate(t, size=(op["hl"], op["wl"]), mode="bilinear", align_corners=False).numpy()
        assert np.abs(NR.apply_A(op, x0) - ref).max() <= 1e-15
        assert NR.n_taps(op, xs[2], xs[3]) == (1 if (xs[2] // op["hl"]) % 2 else 2) * (1 if (xs[3] // op["wl"]) % 2 else 2)


# ---- the coefficient tables ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("chain", ["full", "respaced"])
def test_nullspace_coefs(chain):
    from image_diffusion.sde_diffusion import DDPM

    d = DDPM(100) if chain == "full" else _chain()
    T = {k: v.numpy() for k, v in d.host_tables().items()}
    post = np.exp(0.5 * T["posterior_log_variance_clipped"].astype(np.float64))
    post[0] = 0.0
    lam, sig = d.nullspace_coefs(0.0)
    assert lam.dtype == sig.dtype == torch.float32 and tuple(lam.shape) == tuple(sig.shape) == (d.Ns,)
    assert bool((lam == 1).all()) and np.array_equal(sig.numpy(), post.astype(np.float32))
    for sy in (0.05, 0.5, 3.0):
        lam, sig = d.nullspace_coefs(sy)
        l64, s64 = NR.coefs64(T, sy)
        assert np.array_equal(lam.numpy(), l64.astype(np.float32)) and np.array_equal(sig.numpy(), s64.astype(np.float32))
        assert lam[0] == 0 and sig[0] == 0                      # step 0 draws nothing and a noisy measurement is not pasted into the result
        a = T["posterior_mean_coef1"].astype(np.float64)
        # the variance carried in by the measurement and the variance drawn add up to the posterior's
        assert np.abs((a * l64 * sy) ** 2 + s64 ** 2 - post ** 2)[1:].max() <= 1e-15
    lam, sig = d.nullspace_coefs(3.0)      # a measurement far noisier than the late (low-noise, small i) steps' posterior: lam < 1 and nothing drawn there
    damped = (lam < 1).numpy()
    assert damped[:3].all() and bool((sig[damped] == 0).all()) and bool((lam[1:] > 0).all())
    assert not damped.all() and bool((sig[~damped] > 0).all())
    for bad in (-0.1, float("nan"), float("inf"), True):
        with pytest.raises(ValueError):
            d.nullspace_coefs(bad)


# ---- the budget ------------------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,shape", [(0, s) for s in MASK_SHAPES] + [(k, s) for k in (1, 2) for s in BAND_SHAPES])
def test_fp32_restatement_stays_inside_the_budget(kind, shape):
    worst = 0.0
    for j, (k, f0, f1) in enumerate(step_cases()):
        for pred in PREDS:
            for form, c in ((0, f0), (1, f1)):
                x, out, y, z, op = ns_operands(kind, shape, pred, c, 1000 * j + 10 * form + len(pred))
                zz = z if k > 0 else None
                want, bound = ns_budget(op, pred, form, x, out, y, zz, c)
                got = NR.step32(op, pred, form, x, out, y, zz, c)
                ratio, nan = _ratio(got, want, bound)
                # the planted NaN poisons exactly the taps of its own row (kinds 1, 2; itself where it is no tap) resp. itself (kind 0)
                src = np.isnan(out if pred == "x0" else x)
                own = NR.spread(op, NR.apply_A(op, src.astype(np.float64)), x.shape) > 0 if kind else src
                assert np.array_equal(nan, own | src)
                assert 1 <= nan.sum() <= NR.n_taps(op, x.shape[2], x.shape[3]) + 1
                worst = max(worst, ratio)
                assert ratio <= 1.0, (kind, shape, k, pred, form, ratio)
    print(f"kind {kind}, {shape}: fp32 restatement, worst error / budget {worst:.3f}")


def test_lam_zero_is_the_plain_step():
    """x0 - 0 * r is x0 on finite inputs: the fp32 model of the rectified step equals the plain step of tests/ddpm_respace_ref.py's form."""
    for k, f0, f1 in step_cases()[::2]:
        for form, c in ((0, f0), (1, f1)):
            c = dict(c, lam=0.0)
            x, out, y, z, op = ns_operands(1, BAND_SHAPES[1], "eps", c, 77 + k, nan=False)
            got = NR.step32(op, "eps", form, x, out, y, z, c)
            op0, _ = make_op(0, BAND_SHAPES[1], 3)
            op0["known"][:] = False
            plain = NR.step32(op0, "eps", form, x, out, np.full(x.shape, -2.0, np.float32), z, c)
            assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------------------

def test_nullspace_conditioning_and_average_pooling():
    from image_diffusion.conditioning import Conditioning, NullSpace, get_conditioning
    from image_diffusion.likelihoods import AveragePooling, get_likelihood

    assert get_conditioning("null_space") is NullSpace and NullSpace.KEY == "null_space" and issubclass(NullSpace, Conditioning)
    assert NullSpace.PARAMS == ("sigma_y", "eta", "jump_length", "n_resample")
    c = NullSpace(0.0, None, 1, 1)
    assert (c.sigma_y, c.eta, c.jump_length, c.n_resample) == (0.0, None, 1, 1)
    cfg = dict(sigma_y=0.1, eta=None, jump_length=2, n_resample=3)
    c = NullSpace.from_configdict(cfg)
    assert {n: getattr(c, n) for n in NullSpace.PARAMS} == cfg and "sigma_y=0.1" in repr(c)
    good = dict(sigma_y=0.0, eta=0.5, jump_length=1, n_resample=1)
    for bad in (dict(sigma_y=-1.0), dict(sigma_y=float("nan")), dict(eta=-0.5), dict(eta=float("inf")), dict(jump_length=0), dict(n_resample=0),
                dict(jump_length=1.5), dict(sigma_y=0.1, eta=0.5)):
        with pytest.raises(ValueError):
            NullSpace(**dict(good, **bad))
    with pytest.raises(TypeError):
        NullSpace(0.0, None, 1)
    assert get_likelihood("AveragePooling") is AveragePooling
    lik = AveragePooling.from_configdict(dict(factor=4))
    assert lik.factor == (4, 4) and AveragePooling((2, 3)).factor == (2, 3)
    x = torch.randn(3, 2, 8, 12, generator=torch.Generator().manual_seed(1))
    y = lik.sample(x)
    assert torch.equal(y, F.avg_pool2d(x, 4, 4)) and tuple(lik.none_like(x).shape) == (3, 2, 2, 3) and not lik.none_like(x).any()
    torch.testing.assert_close(lik.loss(x, y), torch.zeros(3))
    torch.testing.assert_close(lik.loss(x, y + 0.5), torch.full((3,), 0.25))
    for bad in (0, -2, 1.5, True, (2, 0)):
        with pytest.raises(ValueError):
            AveragePooling(bad)
    with pytest.raises(ValueError, match="multiple"):
        AveragePooling(3).sample(x)


def test_python_refusals():
    from image_diffusion import sampling
    from image_diffusion.conditioning import NullSpace
    from image_diffusion.likelihoods import AveragePooling, HyperResolution, InPainting, LowResolution
    from image_diffusion.sde_diffusion import DDPM

    r = _chain()
    eps = lambda x, i: x   # noqa: E731
    plain, ddim = NullSpace(0.0, None, 1, 1), NullSpace(0.0, 0.5, 1, 1)
    lik = InPainting(patch_size=3, pad_value=-2)
    mk = lambda chain, cnd=plain, **kw: sampling.get_conditional_sample_fn(eps, chain, cnd, lik, **kw)   # noqa: E731
    with pytest.raises(NotImplementedError, match="x0 shaping"):
        mk(r.with_x0_shaping(dynamic_threshold=0.9))
    with pytest.raises(NotImplementedError, match="tiling"):
        mk(r, tiling=sampling.Tiling())
    with pytest.raises(NotImplementedError, match="tiling"):
        mk(r.with_tiling(sampling.Tiling()))
    with pytest.raises(NotImplementedError, match="feature_cache"):
        mk(r, feature_cache=sampling.FeatureCache(interval=2))
    with pytest.raises(NotImplementedError, match="learned-variance"):
        mk(r.with_learned_variance())
    mk(r.with_learned_variance(), ddim)                                 # taken in the DDIM form
    mk(r.with_prediction("v"))
    with pytest.raises(NotImplementedError, match="time_scale"):
        mk(DDPM.from_betas(np.linspace(1e-4, 0.02, 10), time_scale=10.0))
    for what in ("n_corrector", "guidance_scale", "order"):            # correctors, classifier-free guidance, multistep solvers
        odd = NullSpace(0.0, None, 1, 1)
        setattr(odd, what, 2)
        with pytest.raises(NotImplementedError, match=what):
            mk(r, odd)
    odd = NullSpace(0.0, 0.5, 1, 1)
    odd.sigma_y = 0.2                                                   # (the constructor refuses the pair too)
    with pytest.raises(ValueError, match="sigma_y"):
        mk(r, odd)
    xT = torch.zeros(2, 1, 16, 16)
    with pytest.raises(NotImplementedError, match="HyperResolution"):
        sampling.get_conditional_sample_fn(eps, r, plain, HyperResolution(4, 4))(xT, xT)
    with pytest.raises(NotImplementedError, match="LowResolution factor"):
        sampling.get_conditional_sample_fn(eps, r, plain, LowResolution(5, 4))(xT, torch.zeros(2, 1, 5, 4))
    with pytest.raises(NotImplementedError, match="AveragePooling factor"):
        sampling.get_conditional_sample_fn(eps, r, plain, AveragePooling(3))(xT, torch.zeros(2, 1, 5, 5))
    with pytest.raises(NotImplementedError, match="class labels"):
        with sampling.use_ops(_CpuOps()):
            sampling.get_conditional_sample_fn(eps, r, plain, lik)(xT, xT, y=torch.zeros(2, dtype=torch.long))


def test_walk_of_a_jumping_nullspace_sampler():
    from image_diffusion.conditioning import repaint_walk

    assert repaint_walk(6, 2, 2) == [6, 5, 4, 3, 4, 5, 4, 3, 2, 1, 2, 3, 2, 1, 0]
    assert repaint_walk(6, 1, 1) == [6, 5, 4, 3, 2, 1, 0]


# ---- the generic host loop on CPU tensors ----------------------------------------------------------------------------------------------------------------

class _CpuOps:
    """The ops the generic null-space loop asks for, on CPU tensors: the step is the fp32 restatement in the kernel's operation order."""

    def __init__(self):
        self.log = []

    def nullspace_step_(self, op, form, prediction, x, out, y, c_recip, c_recipm1, a, b=0.0, lam=1.0, sigma=0.0, *, sa=0.0, sb=0.0, z=None, philox=None):
        assert philox is None, "the CPU double takes injected noise"
        shape = tuple(x.shape)
        d = dict(kind=int(op.kind))
        if op.kind == 0:
            d["known"] = (y != op.pad_value).numpy()
        else:
            d.update(hl=int(op.h_low), wl=int(op.w_low))
        c = dict(cr=c_recip, crm1=c_recipm1, sa=sa, sb=sb, a=a, b=b, lam=lam, sigma=sigma)
        new = NR.step32(d, prediction, form, x.numpy(), out[:, :shape[1]].numpy(), y.numpy(), None if z is None else z.numpy(), c)
        self.log.append(("down", form, z is not None, float(lam)))
        x.copy_(torch.from_numpy(new))
        return x

    def renoise_(self, x, z, a, b, philox=None):
        self.log.append(("up",))
        return x.mul_(np.float32(a)).add_(z * np.float32(b))

    def clip_(self, x, lo=-1.0, hi=1.0):
        return x.clip_(lo, hi)


def _toy_net(wide=False):
    def net(xi, i):
        k = float(i[0]) if isinstance(i, torch.Tensor) else float(i)
        o = 0.7 * torch.sin(2.5 * xi + 0.3 * k) + 0.2 * xi.roll(1, dims=-1)
        return torch.cat((o, torch.full_like(o, float("nan"))), dim=1) if wide else o

    return net


@pytest.mark.parametrize("case", ["mask", "mask_plus", "pool_walk", "bilinear_ddim", "pool_v", "mask_wide_ddim"])
def test_generic_host_loop_on_cpu_tensors(case):
    from image_diffusion import sampling
    from image_diffusion.conditioning import NullSpace, repaint_walk
    from image_diffusion.likelihoods import AveragePooling, InPainting, LowResolution

    r = _chain()
    pred = "v" if case == "pool_v" else "eps"
    chain = r.with_prediction(pred) if pred != "eps" else r
    wide = case == "mask_wide_ddim"
    if wide:
        chain = chain.with_learned_variance()
    g = torch.Generator().manual_seed(5)
    xT = torch.randn(3, 1, 16, 16, generator=g)
    truth = torch.rand(3, 1, 16, 16, generator=g) * 2 - 1
    draws = [torch.randn(3, 1, 16, 16, generator=g) for _ in range(20)]
    if case.startswith("mask"):
        lik = InPainting(patch_size=6, pad_value=-2)
        y = truth.clone()
        y[:, :, 4:10, 5:11] = -2.0
        op = dict(kind=0, known=(y != -2.0).numpy())
    elif case.startswith("pool"):
        lik = AveragePooling(4)
        y = lik.sample(truth)
        op = dict(kind=1, hl=4, wl=4)
    else:
        lik = LowResolution(8, 4)
        y = lik.sample(truth)
        op = dict(kind=2, hl=8, wl=4)
    cnd = {"mask": NullSpace(0.0, None, 1, 1), "mask_plus": NullSpace(0.3, None, 1, 1), "pool_walk": NullSpace(0.0, None, 2, 2),
           "bilinear_ddim": NullSpace(0.0, 0.5, 1, 1), "pool_v": NullSpace(0.0, None, 1, 1), "mask_wide_ddim": NullSpace(0.0, 0.0, 1, 1)}[case]
    form = 0 if cnd.eta is None else 1
    net = _toy_net(wide)
    ops = _CpuOps()
    with sampling.use_ops(ops), sampling.injected_noise(draws):
        got = sampling.get_conditional_sample_fn(net, chain, cnd, lik)(xT, y)
    lam, sig = chain.nullspace_coefs(cnd.sigma_y)
    dsig = chain.ddim_sigma(cnd.eta).numpy() if form == 1 and cnd.eta else None
    walk = repaint_walk(r.Ns, cnd.jump_length, cnd.n_resample) if cnd.n_resample > 1 else None
    T = {k: v.numpy() for k, v in chain.host_tables().items()}
    ref, used, n_eval = NR.sample(lambda x, k: net(torch.from_numpy(x), k).numpy(), T, op, pred, form, xT.numpy(), y.numpy(), [d.numpy() for d in draws],
                                  lam.numpy(), sig.numpy(), dsig, walk, channels=1)
    downs = [e for e in ops.log if e[0] == "down"]
    ups = [e for e in ops.log if e[0] == "up"]
    assert len(downs) == n_eval and all(e[1] == form for e in downs)
    assert sum(e[2] for e in downs) + len(ups) == used
    if case == "pool_walk":
        last = sum(1 for a, b in zip(walk, walk[1:]) if (a, b) == (1, 0))                       # step 0 draws nothing
        assert n_eval == 7 + len(ups) and len(ups) == 6 and used == n_eval - last + len(ups)
    if case == "mask_wide_ddim":
        assert used == 0
    if case == "mask_plus":
        assert downs[-1][3] == 0.0 and any(0 < e[3] < 1 for e in downs)
    err = float((got.double() - torch.from_numpy(ref)).abs().max())
    print(f"{case}: host loop on CPU tensors vs the fp64 restatement, max|diff| {err:.3e}")
    assert bool(torch.isfinite(got).all()) and float((got - xT).abs().max()) > 1e-2
    torch.testing.assert_close(got.double(), torch.from_numpy(ref), **STOL)
    if case == "mask":      # plain DDNM: the known pixels of the result are the measurement (lam_0 = 1, coef1_0 = 1, coef2_0 = 0)
        known = torch.from_numpy(op["known"])
        c1 = float(T["posterior_mean_coef1"][0])
        assert float(((got - y).abs() - (4 * EPS32 * (1 + y.abs()) + abs(c1 - 1) * y.abs()))[known].max()) <= 0


# ---- the library: symbols and the refusals that need no device ------------------------------------------------------------------------------------------

def test_library_symbols_and_host_refusals():
    import __graft_entry__ as ge

    ge.build()
    from mi355 import _lib

    L = _lib.lib()
    for name in ("mi355_nullspace_step", "mi355_block_mean", "mi355_ddpm_nullspace_workspace_bytes", "mi355_ddpm_nullspace_sample"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert [f for f, _ in _lib.NullspaceOpC._fields_] == ["kind", "pad_value", "h_low", "w_low"]
    assert [f for f, _ in _lib.NullspaceScheduleC._fields_] == ["lam", "sigma"]
    err = lambda: L.mi355_last_error().decode()   # noqa: E731

    def step(op, form=0, pred=0, batch=0, h=8, w=12, lam=1.0, sigma=0.0, offset=0, stride=0):
        return L.mi355_nullspace_step(C.byref(op) if op is not None else None, form, pred, None, None, stride, None, None, batch, 2, h, w, 1.0, 1.0, 0.0,
                                      0.0, 1.0, 0.0, lam, sigma, 0, 0, offset, None)

    O = _lib.NullspaceOpC
    assert step(O(1, 0.0, 4, 3)) == 0 and step(O(0, -2.0, 0, 0)) == 0 and step(O(2, 0.0, 8, 12)) == 0        # batch = 0: nothing to do
    for op, code, word in ((None, -1, "op is null"), (O(3, 0.0, 4, 3), -1, "op->kind"), (O(-1, 0.0, 4, 3), -1, "op->kind"),
                           (O(1, 0.0, 0, 3), -1, "h_low"), (O(2, 0.0, 4, -1), -1, "w_low"), (O(1, 0.0, 3, 3), -4, "integer factors"),
                           (O(2, 0.0, 4, 5), -4, "integer factors")):
        assert step(op) == code and word in err(), (code, word, err())
    assert step(O(1, 0.0, 1, 2), h=33, w=66) == -4 and "1..32" in err()
    assert step(O(1, 0.0, 1, 2), h=32, w=64) == 0
    good = O(1, 0.0, 4, 3)
    for kw, word in ((dict(form=2), "form"), (dict(pred=3), "pred_kind"), (dict(lam=-0.1), "lam"), (dict(lam=1.5), "lam"), (dict(lam=float("nan")), "lam"),
                     (dict(sigma=-1.0), "sigma"), (dict(sigma=float("inf")), "sigma"), (dict(offset=6), "multiple of 4"), (dict(stride=5), "out_stride"),
                     (dict(batch=-1), "batch")):
        assert step(good, **kw) == -1 and word in err(), (kw, err())
    assert step(good, batch=1) == -1 and "null argument" in err()                                        # with work to do, the pointers are needed
    assert L.mi355_block_mean(None, None, 0, 8, 12, 4, 3, None) == 0
    assert L.mi355_block_mean(None, None, 0, 8, 12, 3, 3, None) == -4 and L.mi355_block_mean(None, None, 0, 8, 12, 0, 3, None) == -1
    assert L.mi355_block_mean(None, None, 2, 8, 12, 4, 3, None) == -1 and "null argument" in err()
    assert L.mi355_ddpm_nullspace_workspace_bytes(None, 3) == -1
    # the loop's refusals that come before the handle is read
    K = 3
    fl = lambda *v: (C.c_float * K)(*v)   # noqa: E731
    arrs = {n: fl(0.5, 0.5, 0.5) for n, _ in _lib.DDPMTablesC._fields_[1:]}
    tb = _lib.DDPMTablesC(K, *[C.cast(arrs[n], C.POINTER(C.c_float)) for n, _ in _lib.DDPMTablesC._fields_[1:]])
    lam_ok, sig_ok = fl(1, 1, 0), fl(0.1, 0.1, 0)
    FP = C.POINTER(C.c_float)

    def loop(mode=_lib.DDPM_PRIOR, y=1, op=good, ns=True, lam=lam_ok, sigma=sig_ok, n_corrector=0, pred=None):
        opt = _lib.DDPMOptionsC(mode, n_corrector, 0.1, 1e-5, 1.0, 1.0, 1, -2.0, -2.0, 0, 0)
        nsc = _lib.NullspaceScheduleC(C.cast(lam, FP) if lam is not None else None, C.cast(sigma, FP) if sigma is not None else None)
        return L.mi355_ddpm_nullspace_sample(None, None, 1, C.c_void_p(256) if y else None, C.byref(op) if op is not None else None, None, C.byref(tb),
                                             C.byref(opt), None, C.byref(nsc) if ns else None, C.byref(pred) if pred is not None else None, None, 0, 3,
                                             None, 0, None)

    for kw, word in ((dict(y=0), "y is null"), (dict(op=None), "op is null"), (dict(ns=False), "ns is null"),
                     (dict(mode=_lib.DDPM_AMORTIZED), "opt->mode"), (dict(mode=_lib.DDPM_REPLACEMENT), "opt->mode"), (dict(n_corrector=1), "n_corrector"),
                     (dict(sigma=None), "ns->sigma is null"), (dict(mode=_lib.DDIM), "ns->sigma given in form 1"), (dict(lam=None), "ns->lam is null"),
                     (dict(lam=fl(1, -0.5, 0)), "ns->lam"), (dict(lam=fl(1, float("nan"), 0)), "ns->lam"), (dict(lam=fl(1, 1.25, 0)), "<= 1"),
                     (dict(sigma=fl(0.1, -0.1, 0)), "ns->sigma"), (dict(sigma=fl(0.1, float("inf"), 0)), "ns->sigma"),
                     (dict(pred=_lib.DDPMPredictionC(3)), "pred->kind")):
        assert loop(**kw) == -1 and word in err(), (kw, err())
    assert loop() == -1 and "bad argument (net, x, workspace, batch)" in err()                           # every host check passed: the handle is next
    assert loop(mode=_lib.DDIM, sigma=None) == -1 and "bad argument (net" in err()
