"""Sampler selectors (what `AD/image_diffusion/conditioning.py:12-78` provides): each type only carries the hyper-parameters
of one conditional sampler; `image_diffusion.sampling` dispatches on the type.

Declarative layout: a subclass names its parameters once in `PARAMS` (in the reference's positional order); construction
from positionals / keywords and from a config mapping are derived from that list.
"""
from typing import Dict, Tuple, Type


class Conditioning:
    PARAMS: Tuple[str, ...] = ()
    KEY: str = ""

    def __init__(self, *args, **kwargs):
        names = self.PARAMS
        if len(args) > len(names):
            raise TypeError(f"{type(self).__name__} takes {len(names)} parameters ({', '.join(names)})")
        given = dict(zip(names, args))
        for k, v in kwargs.items():
            if k not in names or k in given:
                raise TypeError(f"{type(self).__name__}: unexpected or repeated parameter {k!r}")
            given[k] = v
        missing = [n for n in names if n not in given]
        if missing:
            raise TypeError(f"{type(self).__name__}: missing {', '.join(missing)}")
        for n in names:
            setattr(self, n, given[n])

    @classmethod
    def from_configdict(cls, config):
        return cls(**{n: config[n] for n in cls.PARAMS})

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{n}={getattr(self, n)!r}' for n in self.PARAMS)})"


class Amortized(Conditioning):
    """Condition concatenated on the channel axis of the network input; optional Langevin corrector (sampling.py:80-133)."""
    KEY, PARAMS = "amortized", ("p_cond", "n_corrector", "delta")


class ClassifierFreeGuidance(Amortized):
    """Amortized sampling with classifier-free guidance of the predictor: eps = eps_u + guidance_scale * (eps_c - eps_u), eps_u the net fed
    likelihood.none_like (what p_cond's condition dropout trains, loss_functions.py:47-50).  No reference counterpart: the reference trains
    for it and never samples with it."""
    KEY, PARAMS = "classifier_free_guidance", Amortized.PARAMS + ("guidance_scale",)


class ReconstructionGuidance(Conditioning):
    """Gradient guidance through the x0 predictor (sampling.py:136-206): the gradient is the HIP engine's vector-Jacobian product
    (UNetEngine.vjp), so the sampler needs an eps_model made by make_eps_model around a UNetModel."""
    KEY, PARAMS = "reconstruction_guidance", ("gamma", "start_fraction", "update_rule", "n_corrector", "delta")


class Replacement(Conditioning):
    """Known pixels are overwritten by the (optionally re-noised) condition each step (sampling.py:209-260)."""
    KEY, PARAMS = "replacement", ("delta", "start_fraction", "noise", "n_corrector")


class RePaint(Replacement):
    """Replacement with RePaint resampling (Lugmayr et al. 2022): the sampler walks the chain down and, at every jump point, back up
    jump_length levels by the forward move q(x_k | x_{k-1}) and down again, n_resample times in all, which lets the generated pixels
    harmonise with the pasted ones.  The walk is repaint_walk(ddpm.Ns, jump_length, n_resample); n_resample = 1 is Replacement itself.
    Affordable on a respaced chain (DDPM.respace).  No reference counterpart; sample quality is untested."""
    KEY, PARAMS = "repaint", Replacement.PARAMS + ("jump_length", "n_resample")

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if int(self.jump_length) != self.jump_length or self.jump_length < 1:
            raise ValueError(f"jump_length must be an int >= 1, got {self.jump_length!r}")
        if int(self.n_resample) != self.n_resample or self.n_resample < 1:
            raise ValueError(f"n_resample must be an int >= 1, got {self.n_resample!r}")


class NullSpace(Conditioning):
    """Null-space restoration with an unconditional DDPM net (DDNM: Wang, Yu, Zhang, ICLR 2023): every step rectifies its data prediction,
    x0_hat <- x0_hat - lam A^+(A x0_hat - y), for the likelihood's linear operator A (in-/out-painting masks, AveragePooling, LowResolution with an
    integer factor): one evaluation per step, no backward, no step size.  sigma_y: the noise std of the measurement in the data's units (> 0:
    DDNM+, DDPM.nullspace_coefs; the ancestral form only).  eta: None = the ancestral form; a number >= 0 = the DDIM(eta) form with
    ddpm.ddim_sigma(eta).  jump_length, n_resample: DDNM's time travel, the walk repaint_walk(ddpm.Ns, jump_length, n_resample); (1, 1) is the
    plain descent.  No reference counterpart; sample quality is untested."""
    KEY, PARAMS = "null_space", ("sigma_y", "eta", "jump_length", "n_resample")

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if isinstance(self.sigma_y, bool) or not (float(self.sigma_y) >= 0.0 and float(self.sigma_y) < float("inf")):
            raise ValueError(f"sigma_y must be finite and >= 0, got {self.sigma_y!r}")
        if self.eta is not None and (isinstance(self.eta, bool) or not (float(self.eta) >= 0.0 and float(self.eta) < float("inf"))):
            raise ValueError(f"eta must be None (the ancestral form) or a finite number >= 0, got {self.eta!r}")
        if self.eta is not None and float(self.sigma_y) > 0.0:
            raise ValueError("sigma_y > 0 (DDNM+) belongs to the ancestral form: eta must be None")
        if int(self.jump_length) != self.jump_length or self.jump_length < 1:
            raise ValueError(f"jump_length must be an int >= 1, got {self.jump_length!r}")
        if int(self.n_resample) != self.n_resample or self.n_resample < 1:
            raise ValueError(f"n_resample must be an int >= 1, got {self.n_resample!r}")


def repaint_walk(K: int, jump_length: int, n_resample: int):
    """The levels a RePaint sampler visits on a K-step chain: a restatement of the jump schedule of Lugmayr et al. 2022 (their
    get_schedule_jump with jump_n_sample = n_resample).  Level L in [0, K] is the state before step L - 1 is applied; K is noise, 0 the result.
        budget[t] = n_resample - 1 for t in range(0, K - jump_length, jump_length)
        t = K
        while t >= 1:
            t -= 1; emit t
            if budget.get(t, 0) > 0: budget[t] -= 1; repeat jump_length times: t += 1; emit t
    The levels are every emitted t + 1 (the first one is K itself: their t indexes the state x_t, which is level t + 1 here), and the walk
    ends at level 0.  Consecutive levels differ by one: a move down is a sampling step, a move up one re-noising.  n_resample = 1 is the plain
    descent K, K-1, ..., 0; K = 6, jump_length = 2, n_resample = 2 makes 10 steps down and 4 up."""
    K, j, r = int(K), int(jump_length), int(n_resample)
    if K < 1 or j < 1 or r < 1:
        raise ValueError("repaint_walk needs K >= 1, jump_length >= 1 and n_resample >= 1")
    budget = {t: r - 1 for t in range(0, K - j, j)}
    levels = []
    t = K
    while t >= 1:
        t -= 1
        levels.append(t + 1)
        if budget.get(t, 0) > 0:
            budget[t] -= 1
            for _ in range(j):
                t += 1
                levels.append(t + 1)
    levels.append(0)
    return levels


class FlowReplacement(Conditioning):
    """Replacement for an unconditional flow-matching net (flow_sampling.py): during the first int(n_steps * start_fraction) steps the known
    pixels are put on the straight path, x <- where(known, t y + (1 - t) z, x).  noise: "coupled" (z = the sample's own initial state) or
    "fresh" (a new draw per step).  No reference counterpart."""
    KEY, PARAMS = "flow_replacement", ("start_fraction", "noise")

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if self.noise not in ("coupled", "fresh"):
            raise ValueError(f"noise must be 'coupled' or 'fresh', got {self.noise!r}")


class FlowReconstructionGuidance(Conditioning):
    """Reconstruction guidance for an unconditional flow-matching net (flow_sampling.py): during the first int(n_steps * start_fraction) steps
    x <- x + dt v - dt s_k grad_x loss(x + (1 - t_k) v, y).  schedule: "constant" (s_k = gamma), "one_minus_t" (s_k = gamma (1 - t_k), both
    factors and the product in fp32) or a callable t -> float.  replace: None, "coupled" or "fresh" (FlowReplacement's paste in the same steps;
    painting likelihoods only).  No reference counterpart; the defaults are untested for sample quality."""
    KEY, PARAMS = "flow_reconstruction_guidance", ("gamma", "start_fraction", "schedule", "replace")

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        if not (self.schedule in ("constant", "one_minus_t") or callable(self.schedule)):
            raise ValueError(f"schedule must be 'constant', 'one_minus_t' or a callable t -> float, got {self.schedule!r}")
        if self.replace not in (None, "coupled", "fresh"):
            raise ValueError(f"replace must be None, 'coupled' or 'fresh', got {self.replace!r}")

    def scales(self, t_steps):
        """The guidance scale of every step starting at the times t_steps, as fp32 values (Python floats that are exact fp32 numbers)."""
        import torch

        t = torch.tensor([float(v) for v in t_steps], dtype=torch.float32)
        if callable(self.schedule):
            s = torch.tensor([float(self.schedule(float(v))) for v in t], dtype=torch.float32)
        elif self.schedule == "constant":
            s = torch.full_like(t, float(self.gamma))
        else:
            s = torch.tensor(float(self.gamma), dtype=torch.float32) * (torch.tensor(1.0, dtype=torch.float32) - t)
        return [float(v) for v in s]


def flow_split_index(n_steps: int, start_fraction: float) -> int:
    """How many of a flow sampler's n_steps steps, from the noise end, are conditioned: int(n_steps * start_fraction)."""
    return int(n_steps * start_fraction)


_REGISTRY: Dict[str, Type[Conditioning]] = {c.KEY: c for c in (Amortized, ClassifierFreeGuidance, ReconstructionGuidance, Replacement, RePaint,
                                                               NullSpace, FlowReplacement, FlowReconstructionGuidance)}


def get_conditioning(type_: str) -> Type[Conditioning]:
    try:
        return _REGISTRY[type_.lower()]
    except KeyError:
        raise NotImplementedError(f"Unknown conditioning {type_}") from None
