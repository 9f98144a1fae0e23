"""Adaptive Dormand-Prince 5(4) ("dopri5") on the HIP backend.

The reference's default FID solver and all mnist/ evaluations call `torchdiffeq.odeint(f, x, t, rtol, atol,
method="dopri5")` (cifar10/compute_fid.py:80-85, mnist/utils_mnist.py:63-68,101-108, utils_mnist_hy.py:84-92).
torchdiffeq is not vendored (version unpinned); its published algorithm (rk_common.py / dopri5.py / interp.py /
misc.py of the 0.2.x line) is restated here: Hairer initial step, FSAL Dormand-Prince stages, RMS error norm
(max over components for tuple states), accept iff ratio <= 1, step factor min(10, max(0.9 / ratio**(1/5), 0.2))
with the lower bound lifted to 1 on accepted steps, quartic dense output at the requested time.
No reference test pins it: "parity unpinned"; checked against oracle/cfm_ref.dopri5 (same restatement, PyTorch-CPU) and, without a
shared source, against the order conditions of the tables, an analytic solution and scipy's RK45 (tests/test_dopri5_cpu.py).

Stage combinations, error norms and the dense output are HIP kernels (csrc/ode.hip); the controller needs one
scalar per step and stays on the host.
"""
from __future__ import annotations

import math
from typing import Callable, List, Sequence

import torch
import torch.distributed as dist

from .ops import default_ops

ALPHA = [1 / 5, 3 / 10, 4 / 5, 8 / 9, 1.0, 1.0]
BETA = [
    [1 / 5],
    [3 / 40, 9 / 40],
    [44 / 45, -56 / 15, 32 / 9],
    [19372 / 6561, -25360 / 2187, 64448 / 6561, -212 / 729],
    [9017 / 3168, -355 / 33, 46732 / 5247, 49 / 176, -5103 / 18656],
    [35 / 384, 0.0, 500 / 1113, 125 / 192, -2187 / 6784, 11 / 84],
]
C_ERROR = [35 / 384 - 1951 / 21600, 0.0, 500 / 1113 - 22642 / 50085, 125 / 192 - 451 / 720, -2187 / 6784 - -12231 / 42400,
           11 / 84 - 649 / 6300, -1.0 / 60.0]
C_MID = [6025192743 / 30085553152 / 2, 0.0, 51252292925 / 65400821598 / 2, -2691868925 / 45128329728 / 2,
         187940372067 / 1594534317056 / 2, -1776094331 / 19743644256 / 2, 11237099 / 235043384 / 2]

State = List[torch.Tensor]


class Dopri5:
    def __init__(self, func: Callable[[float, State], Sequence[torch.Tensor]], rtol: float, atol: float, ops=None,
                 safety=0.9, ifactor=10.0, dfactor=0.2, max_num_steps=100000, sync_norm=True, dtype=torch.float32):
        """dtype: the state's type.  The HIP ops are fp32; the CPU tests measure the tables' orders with an fp64 op table."""
        self.func, self.rtol, self.atol = func, float(rtol), float(atol)
        self.ops = ops or default_ops
        self.safety, self.ifactor, self.dfactor, self.max_num_steps = safety, ifactor, dfactor, max_num_steps
        self.nfe = 0
        self.n_steps = 0        # attempted steps, rejected ones included: nfe == 6 * n_steps + 2
        self.n_rejected = 0
        self.dtype = dtype
        self.sync_norm = sync_norm

    # ---- helpers -----------------------------------------------------------------------------------------
    def _f(self, t: float, y: State) -> State:
        self.nfe += 1
        return [v.to(self.dtype).contiguous() for v in self.func(t, y)]

    def _norm(self, a: State, sub=None, b=None, b2=None, atol=1.0, rtol=0.0) -> float:
        """max over components of rms((a - sub) / (atol + rtol * max(|b|, |b2|)))  (torchdiffeq _mixed_norm / _rms_norm)."""
        accs = torch.zeros(len(a), dtype=torch.float64, device=a[0].device)
        for i in range(len(a)):
            self.ops.rk_sqnorm(accs[i:i + 1], a[i], sub[i] if sub else None, b[i] if b else None, b2[i] if b2 else None, atol, rtol)
        counts = [float(a[i].numel()) for i in range(len(a))]
        if self.sync_norm and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            # batch sharded over ranks: the reference's norm runs over the WHOLE batch, so the per-step scalar is the one
            # real exchange of this path - a 2*len(state)-double all-reduce per norm keeps every rank on the same steps
            vec = torch.cat([accs, torch.tensor(counts, dtype=torch.float64, device=accs.device)])
            dist.all_reduce(vec)
            accs, counts = vec[: len(a)], vec[len(a):].tolist()
        vals = accs.tolist()  # one host sync per norm (the controller needs the scalar)
        return max(math.sqrt(v / counts[i]) for i, v in enumerate(vals))

    def _combine(self, y0: State, ks: List[State], coeffs: Sequence[float]) -> State:
        out = [torch.empty_like(k) for k in ks[0]]
        for i in range(len(y0)):
            self.ops.rk_combine(out[i], y0[i], [k[i] for k in ks], coeffs)
        return out

    def _initial_step(self, t0: float, y0: State, f0: State) -> float:
        """misc.py _select_initial_step with order = 4."""
        d0 = self._norm(y0, b=y0, atol=self.atol, rtol=self.rtol)
        d1 = self._norm(f0, b=y0, atol=self.atol, rtol=self.rtol)
        h0 = 1e-6 if (d0 < 1e-5 or d1 < 1e-5) else 0.01 * d0 / d1
        y1 = self._combine(y0, [f0], [h0])
        f1 = self._f(t0 + h0, y1)
        d2 = self._norm(f1, sub=f0, b=y0, atol=self.atol, rtol=self.rtol) / h0
        if d1 <= 1e-15 and d2 <= 1e-15:
            h1 = max(1e-6, h0 * 1e-3)
        else:
            h1 = (0.01 / max(d1, d2)) ** (1.0 / 5.0)
        return min(100 * h0, h1)

    # ---- one step ----------------------------------------------------------------------------------------------
    def _step(self, t: float, dt: float, y0: State, f0: State):
        """One Dormand-Prince step from (t, y0) with f0 = f(t, y0) -> (y1, f1, err, ks): the 5th-order state, f(t + dt, y1) (FSAL:
        the last stage), the embedded error estimate and the 7 stage derivatives."""
        t1 = t + dt
        ks = [f0]
        yi = None
        for a, beta in zip(ALPHA, BETA):
            ti = t1 if a == 1.0 else t + a * dt
            yi = self._combine(y0, ks, [b * dt for b in beta])
            ks.append(self._f(ti, yi))
        err = self._combine([None] * len(y0), ks, [c * dt for c in C_ERROR])
        return yi, ks[-1], err, ks                                   # FSAL: c_sol == beta[-1]

    def _midpoint(self, y0: State, ks: List[State], dt: float) -> State:
        return self._combine(y0, ks, [c * dt for c in C_MID])

    def _dense(self, interp, t_eval: float) -> State:
        """interp = (y0, y1, ymid, f0, f1, t0, dt) of an accepted step -> the quartic dense output at t_eval."""
        ya, yb, ym, fa, fb, ta, dta = interp
        out = [torch.empty_like(v) for v in ya]
        for i in range(len(ya)):
            self.ops.rk_interp(out[i], ya[i], yb[i], ym[i], fa[i], fb[i], dta, (t_eval - ta) / dta)
        return out

    # ---- integration ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def integrate_times(self, y0: Sequence[torch.Tensor], times: Sequence[float]) -> List[State]:
        """States at times[1:], one continuous adaptive solve with dense output (torchdiffeq: _before_integrate once,
        then per output time `while next_t > t1: step` followed by `_interp_evaluate`)."""
        y0 = [v.detach().to(self.dtype).contiguous() for v in y0]
        t = float(times[0])
        f0 = self._f(t, y0)
        dt = self._initial_step(t, y0, f0)
        interp = None
        outs: List[State] = []
        for t_end in [float(v) for v in times[1:]]:
            while t_end > t:
                if self.n_steps >= self.max_num_steps:
                    raise RuntimeError("dopri5: max_num_steps exceeded")
                self.n_steps += 1
                y1, f1, err, ks = self._step(t, dt, y0, f0)
                ratio = self._norm(err, b=y0, b2=y1, atol=self.atol, rtol=self.rtol)
                if ratio <= 1.0:
                    interp = (y0, y1, self._midpoint(y0, ks, dt), f0, f1, t, dt)
                    t, y0, f0 = t + dt, y1, f1
                else:
                    self.n_rejected += 1
                if ratio == 0.0:
                    factor = self.ifactor
                else:
                    dfac = 1.0 if ratio < 1.0 else self.dfactor
                    factor = min(self.ifactor, max(self.safety / ratio ** 0.2, dfac))
                dt = dt * factor
            if interp is None:      # requested time equals the start time
                outs.append([v.clone() for v in y0])
                continue
            outs.append(self._dense(interp, t_end))
        return outs

    def integrate(self, y0: Sequence[torch.Tensor], t0: float, t_end: float) -> State:
        return self.integrate_times(y0, [t0, t_end])[-1]


def odeint_dopri5(func, y0, t0: float, t_end: float, rtol: float, atol: float):
    """Single-tensor or tuple state; returns (state at t_end in the input's structure, nfe)."""
    is_tuple = isinstance(y0, (tuple, list))
    ys = list(y0) if is_tuple else [y0]
    f = (lambda t, y: func(t, tuple(y))) if is_tuple else (lambda t, y: [func(t, y[0])])
    solver = Dopri5(f, rtol, atol)
    out = solver.integrate(ys, t0, t_end)
    return (tuple(out) if is_tuple else out[0]), solver.nfe
