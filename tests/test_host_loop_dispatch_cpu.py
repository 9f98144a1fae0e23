"""CPU: what every Python DDPM sampler of image_diffusion/sampling.py does with an eps_model - on the host-loop path (any callable) the ops it calls
and in which order, with which scalars, tensor operands, noise draws and guidance scales, and the evaluations it asks of the eps_model; on the fused
path (an eps_model tagged by make_eps_model) the engine method it picks and every argument and keyword that method receives.  Nothing runs on a
device: the op table is a recording double installed with sampling.use_ops, the eps_model a recording callable, the engine a recording object (the
pattern of tests/test_engine_dispatch_cpu.py, one level higher).

The op double.  Every op the loops call is answered by one generic recorder: the call is bound to the real mi355.ops.Ops signature (so a value given
by position, by keyword or left at its default is the same row), and the row holds the op name and every argument - strings and scalars as their exact
repr, tensors as shape, dtype and a content hash, z given or not, the philox pair, w as a float or a hash.  An in-place op then overwrites its state with
an integer-valued mix of the state and of a number hashed from the whole row (dpmpp's hist likewise); cfg_combine and the two shape-stats ops return
such a mix.  A swapped operand or a reordered call therefore changes every later hash.

The eps_model double is untagged, records (step index, input shape, input hash) per call and returns an integer-valued mix of its input, the step and
the call number, of the state's channels (twice as many on a learned-variance chain).  The engine double hangs on a tagged eps_model
(make_eps_model around a fake network) and records the method name, the positional arguments and every keyword as given.  The state handed to a
fused case is a tensor whose is_cuda reads True: the one thing patched, for _fast_engine's test.

The expected rows (tests/golden/host_loop_dispatch.json: per case and run the first 16 hex digits of the SHA-256 of the full transcript, or the
refusal - exception type, message and whether the factory or sample() raised it; every distinct refusal is written out once) are the behaviour when this file was written; a change of the loop
code must leave every row as it is.  `python tests/test_host_loop_dispatch_cpu.py --write` rewrote the file, `--dump FILE` writes the full transcripts
(to compare two trees row by row).
"""
import ctypes
import dataclasses
import functools
import hashlib
import inspect
import itertools
import json
import os
import sys

if __name__ == "__main__":
    _REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_REPO, os.path.join(_REPO, "image-inpainting-and-super-resolution-using-diffusion-models-and-conditional-flow-matching_amd")):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import numpy as np
import pytest
import torch

B, C, S, K = 3, 2, 4, 4   # batch (a per-image w has distinct rows), channels, image size, DDPM steps
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_loop_dispatch.json")
SEED = 1234


# ---- encoding ----------------------------------------------------------------------------------------------------------------------------------------

def _plain_tensor(t):
    return t.detach().as_subclass(torch.Tensor).contiguous()


def enc(v):
    if isinstance(v, torch.Tensor):
        t = _plain_tensor(v)
        return f"T{tuple(t.shape)}:{str(t.dtype)[6:]}:{hashlib.sha256(t.numpy().tobytes()).hexdigest()[:16]}"
    if v is None or isinstance(v, (bool, int, float, str)):
        return repr(v)
    if isinstance(v, (np.integer, np.floating)):
        return f"np:{v!r}"
    if isinstance(v, (tuple, list)):
        return "(" + ",".join(enc(e) for e in v) + ")"
    if isinstance(v, dict):
        return "{" + ",".join(f"{k}={enc(v[k])}" for k in sorted(v)) + "}"
    if isinstance(v, ctypes.Structure):
        return type(v).__name__ + enc(tuple(getattr(v, f) for f, _ in v._fields_))
    if dataclasses.is_dataclass(v):
        return repr(v)
    return type(v).__name__ + enc(vars(v))


def _mix(t, h):
    """Integer-valued, exact in fp32, depends on every element of t and on h."""
    return torch.remainder(t * 3.0 + float(h), 251.0) - 125.0


# ---- the doubles -------------------------------------------------------------------------------------------------------------------------------------

class OpDouble:
    """Stands where mi355.ops.default_ops stands (sampling.use_ops)."""

    def __init__(self, log):
        self.log = log

    def __getattr__(self, name):
        from mi355.ops import Ops

        sig = inspect.signature(getattr(Ops, name))

        def op(*args, **kwargs):
            bound = sig.bind(None, *args, **kwargs)
            bound.apply_defaults()
            a = dict(bound.arguments)
            a.pop("self")
            # hist goes in by its shape: the loop allocates it uninitialised, and what it holds later is what this double wrote from earlier rows
            row = name + " " + " ".join(f"{k}={enc(tuple(v.shape)) if k == 'hist' and v is not None else enc(v)}" for k, v in a.items())
            self.log.append(row)
            h = int(hashlib.sha256(row.encode()).hexdigest()[:8], 16) % 251
            if name == "cfg_combine":
                v2 = a["v2"]
                n = v2.shape[0] // 2
                return _mix(v2[:n] * 2.0 + v2[n:], h)
            if name in ("x0_shape_stats", "pred_shape_stats"):
                base = torch.remainder(a["x"].flatten(1).sum(1), 17.0)
                return torch.stack((base + float(h % 13), base * 2.0 + float(h % 11)), dim=1)
            x = a["x"]
            if name != "clip_":
                x.copy_(_mix(x, h))
                if a.get("hist") is not None:
                    a["hist"].copy_(_mix(x[:a["hist"].shape[0]] * 7.0, h + 3))
            return x

        return op


def eps_double(log, width):
    calls = itertools.count()

    def eps_model(xi, i):
        n = next(calls)
        step = int(i[0]) if isinstance(i, torch.Tensor) else int(i)
        log.append(f"eval step={step} in={enc(xi)}")
        x = xi.float()
        base = x[:, :C] + (2.0 * x[:, C:2 * C] if x.shape[1] >= 2 * C else 0.0)
        out = _mix(base * 5.0, step + 7 * n)
        return torch.cat((out, _mix(out, 11))[:width // C], dim=1)

    return eps_model


class EngineDouble:
    METHODS = ("ddpm_sample", "ddpm_shaped", "ddpm_learned", "ddpm_pred", "ddpm_multistep", "ddpm_nullspace")

    def __init__(self, log, out_channels):
        self.log, self.out_channels = log, out_channels

    def __getattr__(self, name):
        if name not in self.METHODS:
            raise AttributeError(name)

        def method(*args, **kwargs):
            self.log.append(f"engine.{name} args={enc(args)} " + " ".join(f"{k}={enc(kwargs[k])}" for k in sorted(kwargs)))
            return args[0]

        return method


class NetDouble:
    def __init__(self, engine):
        self._engine = engine

    def engine(self, device, **kw):
        self._engine.log.append(f"net.engine device={device} {enc(kw)}")
        return self._engine

    def __call__(self, x, t):
        raise AssertionError("a fused case never evaluates the network from Python")


class CudaLike(torch.Tensor):
    is_cuda = property(lambda self: True)


# ---- operands ----------------------------------------------------------------------------------------------------------------------------------------

def _ints(seed, *shape):
    return torch.randint(-3, 4, shape, generator=torch.Generator().manual_seed(seed)).float()


def operands():
    xT = _ints(1, B, C, S, S)
    cond = _ints(2, B, C, S, S)
    cond[:, :, 1:3, 1:3] = -2.0
    draws = [_ints(10 + j, B, C, S, S) for j in range(40)]
    return xT, cond, draws


@functools.lru_cache(maxsize=None)
def chains():
    from image_diffusion import sampling
    from image_diffusion.sde_diffusion import DDPM

    base = DDPM.from_betas(np.linspace(0.05, 0.6, K))
    return {
        "plain": base,
        "respaced": DDPM.from_betas(np.linspace(0.02, 0.4, 8)).respace(K),   # 4 of 8 steps
        "shaped_q": base.with_x0_shaping(dynamic_threshold=0.9),
        "shaped_q_rescale": base.with_x0_shaping(dynamic_threshold=0.9, guidance_rescale=0.7),
        "learned": base.with_learned_variance(),
        "x0": base.with_prediction("x0"),
        "v": base.with_prediction("v"),
        "v_learned": base.with_prediction("v").with_learned_variance(),
        "v_shaped": base.with_prediction("v").with_x0_shaping(dynamic_threshold=0.9),
        "learned_shaped": base.with_learned_variance().with_x0_shaping(dynamic_threshold=0.9),
        "learned_large": base.with_learned_variance().with_fixed_variance("large"),
        "time_scale": DDPM.from_betas(np.linspace(0.05, 0.6, K), time_scale=float(K)),
        "time_scale_shaped": DDPM.from_betas(np.linspace(0.05, 0.6, K), time_scale=float(K)).with_x0_shaping(dynamic_threshold=0.9),
        "tiled": base.with_tiling(sampling.Tiling(stride=2)),
        "cached": base.with_feature_cache(sampling.FeatureCache(interval=2)),
        "v_tiled": base.with_prediction("v").with_tiling(sampling.Tiling(stride=2)),
        "learned_cached": base.with_learned_variance().with_feature_cache(sampling.FeatureCache(interval=2)),
        "tiled_cached": base.with_tiling(sampling.Tiling(stride=2)).with_feature_cache(sampling.FeatureCache(interval=2)),
    }


@functools.lru_cache(maxsize=None)
def samplers():
    """name -> (factory(eps_model, chain), call(sample, xT, cond)); the factory runs first, on its own, so that a refusal says where it was raised."""
    from image_diffusion import sampling as sp
    from image_diffusion.conditioning import Amortized, ClassifierFreeGuidance, NullSpace, RePaint, Replacement
    from image_diffusion.likelihoods import AveragePooling, InPainting

    lik = InPainting(patch_size=2, pad_value=-2.0)
    pool = AveragePooling(2)
    wt = torch.tensor([0.5, 1.5, 2.5])
    prior = lambda s, x, c: s(x)                    # noqa: E731
    condl = lambda s, x, c: s(x, c)                 # noqa: E731
    alone = lambda s, x, c: s(x)                    # noqa: E731
    pooled = lambda s, x, c: s(x, pool.sample(c))   # noqa: E731

    def guided_direct(e, d, x, c):
        """The guided ancestral loop with a corrector and a per-image w, which ClassifierFreeGuidance's float() does not let through: the loops
        themselves (what tests/test_gpu_learned_variance.py calls)."""
        engine = sp._fast_engine(e, d, x)
        if engine is not None:
            return sp._run_fast(engine, d, x, sp._lib.DDPM_AMORTIZED, c, n_corrector=1, delta=0.1, none_value=-2.0, guidance_scale=wt)
        return sp._run_generic_cfg(e, d, x, cond=c, none=lik.none_like(x), guidance_scale=wt, n_corrector=1, delta=0.1)

    out = {
        "prior_unconditional": (lambda e, d: sp.get_prior_sample_fn(e, d, Replacement(0.1, 1.0, True, 0), lik), prior),
        "prior_amortized": (lambda e, d: sp.get_prior_sample_fn(e, d, Amortized(0.1, 0, 0.1), lik), prior),
        "prior_cache_argument": (lambda e, d: sp.get_prior_sample_fn(e, d, Amortized(0.1, 0, 0.1), lik, feature_cache=sp.FeatureCache(schedule=[1, 0, 1, 0])), prior),
        "amortized": (lambda e, d: sp.get_conditional_sample_fn(e, d, Amortized(0.1, 0, 0.1), lik), condl),
        "amortized_corrector": (lambda e, d: sp.get_conditional_sample_fn(e, d, Amortized(0.1, 1, 0.25), lik), condl),
        "amortized_tiling_argument": (lambda e, d: sp.get_conditional_sample_fn(e, d, Amortized(0.1, 0, 0.1), lik, tiling=sp.Tiling(stride=1, weight="tent")), condl),
        "replacement_noisy": (lambda e, d: sp.get_conditional_sample_fn(e, d, Replacement(0.1, 0.6, True, 0), lik), condl),
        "replacement_clean_corrector": (lambda e, d: sp.get_conditional_sample_fn(e, d, Replacement(0.2, 0.6, False, 1), lik), condl),
        "repaint_walk": (lambda e, d: sp.get_conditional_sample_fn(e, d, RePaint(0.1, 0.6, True, 0, 1, 2), lik), condl),
        "repaint_descent": (lambda e, d: sp.get_conditional_sample_fn(e, d, RePaint(0.1, 0.6, True, 0, 1, 1), lik), condl),
        "cfg_float_corrector": (lambda e, d: sp.get_conditional_sample_fn(e, d, ClassifierFreeGuidance(0.1, 1, 0.1, 2.0), lik), condl),
        "cfg_tensor_corrector": (lambda e, d: sp.get_conditional_sample_fn(e, d, ClassifierFreeGuidance(0.1, 1, 0.1, wt), lik), condl),
        "guided_direct_tensor_w_corrector": (lambda e, d: (lambda x, c: guided_direct(e, d, x, c)), condl),
        "ddim_eta0": (lambda e, d: sp.get_ddim_sample_fn(e, d, lik), alone),
        "ddim_eta0_condition": (lambda e, d: sp.get_ddim_sample_fn(e, d, lik), condl),
        "ddim_eta05": (lambda e, d: sp.get_ddim_sample_fn(e, d, None, eta=0.5), alone),
        "ddim_eta0_guided": (lambda e, d: sp.get_ddim_sample_fn(e, d, lik, guidance_scale=2.0), condl),
        "ddim_eta05_guided_tensor_w": (lambda e, d: sp.get_ddim_sample_fn(e, d, None, guidance_scale=wt, eta=0.5), condl),
        "ddim_guided_without_condition": (lambda e, d: sp.get_ddim_sample_fn(e, d, lik, guidance_scale=2.0), alone),
        "dpm1": (lambda e, d: sp.get_dpm_solver_sample_fn(e, d, None, order=1), alone),
        "dpm2_likelihood": (lambda e, d: sp.get_dpm_solver_sample_fn(e, d, lik, order=2), alone),
        "dpm2_condition": (lambda e, d: sp.get_dpm_solver_sample_fn(e, d, lik, order=2), condl),
        "dpm1_guided_likelihood": (lambda e, d: sp.get_dpm_solver_sample_fn(e, d, lik, guidance_scale=2.0, order=1), condl),
        "dpm2_guided": (lambda e, d: sp.get_dpm_solver_sample_fn(e, d, None, guidance_scale=wt, order=2), condl),
        "dpm2_guided_without_condition": (lambda e, d: sp.get_dpm_solver_sample_fn(e, d, None, guidance_scale=2.0, order=2), alone),
        "nullspace_ancestral": (lambda e, d: sp.get_conditional_sample_fn(e, d, NullSpace(0.0, None, 1, 1), lik), condl),
        "nullspace_ancestral_plus_walk": (lambda e, d: sp.get_conditional_sample_fn(e, d, NullSpace(0.3, None, 1, 2), lik), condl),
        "nullspace_ddim_eta0": (lambda e, d: sp.get_conditional_sample_fn(e, d, NullSpace(0.0, 0.0, 1, 1), lik), condl),
        "nullspace_ddim_eta05_walk_pool": (lambda e, d: sp.get_conditional_sample_fn(e, d, NullSpace(0.0, 0.5, 1, 2), pool), pooled),
        "nullspace_labels": (lambda e, d: sp.get_conditional_sample_fn(e, d, NullSpace(0.0, None, 1, 1), lik),
                             lambda s, x, c: s(x, c, y=torch.tensor([1, 0, 2]))),
    }
    return out


def case_ids():
    return [f"{s}|{c}" for s in samplers() for c in chains()]


# ---- one case ----------------------------------------------------------------------------------------------------------------------------------------

def transcript(sampler, chain_name, fused, injected):
    """-> the rows of one run: a refusal, or every call in order and the hash of what sample() returned."""
    from image_diffusion import sampling

    factory, call = samplers()[sampler]
    chain = chains()[chain_name]
    xT, cond, draws = operands()
    log = []
    width = C * (2 if getattr(chain, "learned_variance", False) else 1)
    if fused:
        eps_model = sampling.make_eps_model(NetDouble(EngineDouble(log, width)), chain)
        xT = xT.as_subclass(CudaLike)
    else:
        eps_model = eps_double(log, width)
    saved = sampling._draw_counter, sampling._noise_offset
    sampling._draw_counter, sampling._noise_offset = 0, 0
    torch.manual_seed(SEED)
    phase = "factory"
    try:
        sample = factory(eps_model, chain)
        phase = "sample"
        with sampling.use_ops(OpDouble(log)):
            if injected:
                with sampling.injected_noise(draws):
                    got = call(sample, xT, cond)
            else:
                got = call(sample, xT, cond)
        log.append(f"returned {enc(got)} draw_counter={sampling._draw_counter} noise_offset={sampling._noise_offset}")
    except Exception as e:   # the row of a refused pair
        log.append(f"refused {type(e).__name__} at={phase} message={str(e)!r}")
    finally:
        sampling._draw_counter, sampling._noise_offset = saved
    return log


def _short(rows):
    """The sequence of calls in short: runs of one name collapsed."""
    names = [r.split(" ", 1)[0] for r in rows if not r.startswith(("returned", "refused"))]
    return " ".join(f"{n}x{len(list(g))}" for n, g in itertools.groupby(names))


KEYS = ("host/injected", "host/philox", "fused/injected", "fused/philox")


@functools.lru_cache(maxsize=None)
def observe(case):
    """-> per key of KEYS (the sequence of calls in short, the refusal row or the SHA-256 of the transcript)."""
    sampler, chain_name = case.split("|")
    out = {}
    for key in KEYS:
        rows = transcript(sampler, chain_name, key.startswith("fused"), key.endswith("injected"))
        out[key] = (_short(rows), rows[-1] if rows[-1].startswith("refused") else hashlib.sha256("\n".join(rows).encode()).hexdigest()[:16])
    return out


def load_golden():
    """The file holds every distinct refusal row once and, per sampler and chain form, one token per key of KEYS: the first 16 hex digits of the
    transcript's SHA-256, or r<n> for refusal n.  -> case -> the four expected values"""
    with open(GOLDEN) as f:
        g = json.load(f)
    return {f"{s}|{c}": [g["refusals"][int(t[1:])] if t.startswith("r") else t for t in toks.split()] for s, row in g["cases"].items() for c, toks in row.items()}


def write_golden():
    seen = {c: [observe(c)[k][1] for k in KEYS] for c in case_ids()}
    refusals = sorted({v for vs in seen.values() for v in vs if v.startswith("refused")})
    with open(GOLDEN, "w") as f:
        f.write('{"refusals": [\n' + ",\n".join(json.dumps(r) for r in refusals) + '\n],\n"cases": {\n')
        f.write(",\n".join(json.dumps(s) + ": " + json.dumps({c: " ".join(f"r{refusals.index(v)}" if v.startswith("refused") else v for v in seen[f"{s}|{c}"])
                                                                  for c in chains()}) for s in samplers()))
        f.write("\n}}\n")


# ---- the tests ---------------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def expect():
    return load_golden()


def test_every_case_is_expected_and_every_path_is_reached(expect):
    assert sorted(expect) == sorted(case_ids())
    calls = " ".join(v[0] for c in case_ids() for v in observe(c).values())
    for op in ("ddpm_step_", "ddim_step_", "ddim_eta_step_", "dpmpp_step_", "corrector_step_", "x0_shaped_step_", "strided_step_", "ddpm_lv_step_",
               "pred_step_", "cfg_combine", "renoise_", "replace_mask_", "x0_shape_stats", "pred_shape_stats", "nullspace_step_", "clip_", "eval") + \
            tuple("engine." + m for m in EngineDouble.METHODS):
        assert op + "x" in calls, f"no case reaches {op}"
    refusals = [v for e in expect.values() for v in e if v.startswith("refused")]
    assert any("at=factory" in r for r in refusals) and any("at=sample" in r for r in refusals)


@pytest.mark.parametrize("case", case_ids())
def test_dispatch(case, expect):
    got = observe(case)
    for key, want in zip(KEYS, expect[case]):
        if got[key][1] != want:
            sampler, chain_name = case.split("|")
            rows = transcript(sampler, chain_name, key.startswith("fused"), key.endswith("injected"))
            raise AssertionError(f"{case} {key}: expected {want}, got {got[key][1]}; the rows now:\n" + "\n".join(rows))


if __name__ == "__main__":
    if sys.argv[1:2] == ["--write"]:
        write_golden()
    elif sys.argv[1:2] == ["--dump"]:
        with open(sys.argv[2], "w") as f:
            for c in case_ids():
                s, d = c.split("|")
                for key in KEYS:
                    f.write(f"==== {c} {key}\n")
                    f.write("\n".join(transcript(s, d, key.startswith("fused"), key.endswith("injected"))) + "\n")
    else:
        sys.exit(__doc__)
