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

Fixed-step explicit Runge-Kutta methods (`TABLEAUS`, `FixedStepRK`): the solvers behind torchdyn's NeuralODE(solver=...) and the
reference's --integration_method beyond "euler".  One step per interval of the time grid (torchdyn's meaning of t_span).  A tableau is
(a, b, c): a the square stage matrix, row-major, strictly lower triangular; step k with dt = t_{k+1} - t_k evaluates
k_i = f(T_i, y + sum_{j<i} dt a_ij k_j) and ends at y + sum_j dt b_j k_j.  The stage time T_i is t_k for c_i == 0, t_{k+1} itself for c_i == 1
(the rule of the dopri5 stages above) and t_k + c_i * dt otherwise, each operation rounded in the state's type.  Zero coefficients are
skipped.  The same rule runs inside the library as mi355_cfm_rk_sample (UNetEngine.cfm_rk: the whole integration in one call);
FixedStepRK is the host-driven loop for any callable and any tuple state, one mi355_rk_stage launch per stage and component.
Which names the un-vendored libraries give these tables is recalled, not checked - "parity unpinned": torchdyn's "rk4" is recalled as the
classical tableau ("rk4" here), torchdiffeq's fixed-grid "rk4" as the 3/8 rule ("rk4_38" here), "midpoint" as the explicit midpoint rule
in both.  The tables themselves are held to their order conditions and a measured convergence order (tests/test_rk_cpu.py).

Adams-Bashforth methods of order 2 to 4 (`AB_SOLVERS`, `ab_weights`, `AdamsBashforth`; no reference counterpart): one evaluation per step
from step order - 1 on, x_{k+1} = x_k + sum_j w_kj v_{k-j} with the weights integrated over the grid as given (variable-step form), after
order - 1 Runge-Kutta start steps (`AB_START`).  The same rule runs inside the library as mi355_cfm_ab_sample (UNetEngine.cfm_ab);
weights, exactness and measured orders: tests/test_multistep_cpu.py.
"""
from __future__ import annotations

import math
from fractions import Fraction as _Fr
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


# ---- fixed-step explicit Runge-Kutta ---------------------------------------------------------------------------------------------------

def _tab(a, b, c):
    n = len(b)
    return ([[_Fr(v) for v in list(r) + [0] * (n - len(r))] for r in a], [_Fr(v) for v in b], [_Fr(v) for v in c])


_h, _t = _Fr(1, 2), _Fr(1, 3)
# name -> (a, b, c), exact rationals (float(.) of each is what the solvers use)
TABLEAUS = {
    "euler": _tab([[]], [1], [0]),
    "midpoint": _tab([[], [_h]], [0, 1], [0, _h]),                                     # explicit midpoint
    "heun2": _tab([[], [1]], [_h, _h], [0, 1]),                                        # explicit trapezoid
    "rk4": _tab([[], [_h], [0, _h], [0, 0, 1]], [_Fr(1, 6), _t, _t, _Fr(1, 6)], [0, _h, _h, 1]),                       # classical
    "rk4_38": _tab([[], [_t], [-_t, 1], [1, -1, 1]], [_Fr(1, 8), _Fr(3, 8), _Fr(3, 8), _Fr(1, 8)], [0, _t, 2 * _t, 1]),   # 3/8 rule
}
RK_SOLVERS = tuple(n for n in TABLEAUS if n != "euler")   # the names NeuralODE(solver=...) and --integration_method add to "euler" / "dopri5"


def resolve_tableau(method):
    """A name of TABLEAUS or an (a, b, c) triple -> (a [s][s], b [s], c [s]) as floats, 1 <= s <= 4 stages (a: rows of any length up to s;
    only the strictly lower part is kept).  Unknown names raise NotImplementedError; a triple that is not explicit, whose weights b are all
    zero or whose c_i differs from sum_j a_ij (beyond 1e-6, room for decimal thirds) raises ValueError."""
    if isinstance(method, str):
        if method not in TABLEAUS:
            raise NotImplementedError(f"method={method!r}: the fixed-step tableaus are {sorted(TABLEAUS)}")
        method = TABLEAUS[method]
    try:
        a, b, c = method
        b, c = [float(v) for v in b], [float(v) for v in c]
        rows = [[float(v) for v in r] for r in a]
    except (TypeError, ValueError) as e:
        raise ValueError("a tableau is a name or an (a, b, c) triple of numbers") from e
    s = len(b)
    if not 1 <= s <= 4:
        raise ValueError(f"a tableau must have 1 to 4 stages, got {s}")
    if len(c) != s or len(rows) != s:
        raise ValueError("a, b and c of a tableau must have one entry (row) per stage")
    if any(v != 0.0 for i, r in enumerate(rows) for v in r[i:]):
        raise ValueError("only explicit methods are built: a must be strictly lower triangular")
    if all(v == 0.0 for v in b):
        raise ValueError("the weights b of a tableau are all zero: such a step leaves the state where it is")
    if any(abs(c[i] - sum(r[:i])) > 1e-6 for i, r in enumerate(rows)):
        raise ValueError("c_i must equal sum_j a_ij: the stage times would not match the stage states")
    return [[r[j] if j < min(i, len(r)) else 0.0 for j in range(s)] for i, r in enumerate(rows)], b, c


class FixedStepRK:
    """Host-driven fixed-step explicit Runge-Kutta integration of y' = func(t, y) for any callable and any tuple state."""

    def __init__(self, func: Callable[[float, State], Sequence[torch.Tensor]], tableau, ops=None, dtype=torch.float32):
        """tableau: a name of TABLEAUS or an (a, b, c) triple.  dtype: the state's type (the HIP op is fp32; the CPU tests measure the
        tables' orders with an fp64 op table)."""
        self.func = func
        self.a, self.b, self.c = resolve_tableau(tableau)
        self.stages = len(self.b)
        self.ops = ops or default_ops
        self.dtype = dtype
        self.nfe = 0

    def _f(self, t: float, y: State) -> State:
        self.nfe += 1
        return [v.to(self.dtype).contiguous() for v in self.func(t, y)]

    def _s(self, v) -> torch.Tensor:
        return torch.tensor(float(v), dtype=self.dtype)   # host scalars are rounded, and combined, in the state's type

    def _stage(self, y: State, ks: List[State], coeffs: Sequence[float], dt: torch.Tensor) -> State:
        """y + sum_j (dt * coeffs[j]) ks[j] over the non-zero coefficients; y itself when there is none."""
        nz = [(k, float(dt * self._s(c))) for k, c in zip(ks, coeffs) if c != 0.0]
        if not nz:
            return y
        out = [torch.empty_like(v) for v in y]
        for i in range(len(y)):
            self.ops.rk_stage(out[i], y[i], [k[i] for k, _ in nz], [c for _, c in nz])
        return out

    @torch.no_grad()
    def integrate_times(self, y0: Sequence[torch.Tensor], times: Sequence[float]) -> List[State]:
        """States at times[1:], one step per interval (the grid may be non-uniform or decreasing)."""
        y = [v.detach().to(self.dtype).contiguous() for v in y0]
        outs: List[State] = []
        for k in range(len(times) - 1):
            t0, t1 = self._s(times[k]), self._s(times[k + 1])
            dt = t1 - t0
            ks: List[State] = []
            for i in range(self.stages):
                ti = t0 if self.c[i] == 0.0 else (t1 if self.c[i] == 1.0 else t0 + self._s(self.c[i]) * dt)
                ks.append(self._f(float(ti), self._stage(y, ks, self.a[i][:i], dt)))
            y1 = self._stage(y, ks, self.b, dt)
            y = y1 if y1 is not y else [v.clone() for v in y]
            outs.append(y)
        return outs

    def integrate(self, y0: Sequence[torch.Tensor], t0: float, t_end: float) -> State:
        return self.integrate_times(y0, [t0, t_end])[-1]


# ---- Adams-Bashforth (fixed grid, variable step) ------------------------------------------------------------------------------------------

AB_SOLVERS = ("ab2", "ab3", "ab4")   # order q = 2, 3, 4: one evaluation per step from step q - 1 on; a table of their own, not TABLEAUS
# the first q - 1 steps: a Runge-Kutta method of local order >= q - 1 (the global order survives) whose first stage sits at t_k (c_1 = 0), so
# that it is v(t_k, x_k), the history sample
AB_START = {"ab2": "euler", "ab3": "midpoint", "ab4": "rk4"}


def _ab_order(method) -> int:
    if method not in AB_SOLVERS:
        raise NotImplementedError(f"method={method!r}: the Adams-Bashforth samplers are {AB_SOLVERS}")
    return AB_SOLVERS.index(method) + 2


def _ab_weights64(t, order: int):
    """ab_weights in fp64 on the fp64 grid t (numpy)."""
    import numpy as np

    if isinstance(order, bool) or order not in (2, 3, 4):
        raise ValueError(f"order must be 2, 3 or 4, got {order!r}")
    if t.size < 1 or not np.isfinite(t).all():
        raise ValueError("t_span must hold finite times")
    d = np.diff(t)
    if d.size and not ((d > 0).all() or (d < 0).all()):
        raise ValueError("t_span must be strictly monotone: the Lagrange nodes of a step must be distinct")
    n = t.size - 1
    w = np.zeros((max(n, 0), order))
    for k in range(order - 1, n):
        nodes = t[k - np.arange(order)] - t[k]            # shifted to t_k = 0: the integral runs over [0, dt]
        dt = t[k + 1] - t[k]
        for j in range(order):
            p = np.poly1d([1.0])
            for m in range(order):
                if m != j:
                    p = p * np.poly1d([1.0, -nodes[m]]) / (nodes[j] - nodes[m])
            w[k, j] = np.polyint(p)(dt)
    return w


def ab_weights(t_span: Sequence[float], order: int) -> torch.Tensor:
    """CPU fp32 [n_steps, order]: row k holds w_kj = the integral over [t_k, t_{k+1}] of the Lagrange basis polynomial of node t_{k-j} among
    t_k, ..., t_{k-order+1} (the step length is inside the weight), so that x_{k+1} = x_k + sum_j w_kj v_{k-j} integrates polynomials of degree
    order - 1 exactly.  Computed in fp64 from the fp32 grid values (what the library sees) and rounded once.  Rows k < order - 1 (start steps)
    are zero.  A grid that is not strictly monotone raises ValueError."""
    import numpy as np

    t = np.asarray([float(v) for v in t_span], dtype=np.float32).astype(np.float64)
    return torch.from_numpy(_ab_weights64(t, order).astype(np.float32))


class AdamsBashforth:
    """Host-driven Adams-Bashforth integration of y' = func(t, y) for any callable and any tuple state, beside FixedStepRK: steps 0..order-2
    by the start method (FixedStepRK's step; its first stage is kept as the history sample), then one evaluation and one mi355_rk_stage
    launch per step and component.  The library runs the same rule as mi355_cfm_ab_sample (UNetEngine.cfm_ab)."""

    def __init__(self, func: Callable[[float, State], Sequence[torch.Tensor]], method="ab2", start=None, ops=None, dtype=torch.float32):
        self.order = _ab_order(method)
        self.rk = FixedStepRK(func, AB_START[method] if start is None else start, ops=ops, dtype=dtype)
        if self.rk.c[0] != 0.0:
            raise ValueError("the start method's first stage must sit at t_k (c_1 == 0): it is the history sample")
        self.ops = self.rk.ops
        self.dtype = dtype

    @property
    def nfe(self) -> int:
        return self.rk.nfe

    @torch.no_grad()
    def integrate_times(self, y0: Sequence[torch.Tensor], times: Sequence[float]) -> List[State]:
        """States at times[1:], one step per interval (the grid may be non-uniform or decreasing, not repeating)."""
        q, rk = self.order, self.rk
        # the weights from the grid as the state's type holds it, rounded to that type (fp32: ab_weights itself)
        w = torch.from_numpy(_ab_weights64(torch.tensor([float(v) for v in times], dtype=self.dtype).double().numpy(), q)).to(self.dtype)
        y = [v.detach().to(self.dtype).contiguous() for v in y0]
        hist: List[State] = []   # v_k, v_{k-1}, ...
        outs: List[State] = []
        for k in range(len(times) - 1):
            if k < q - 1:
                t0, t1 = rk._s(times[k]), rk._s(times[k + 1])
                dt = t1 - t0
                ks: List[State] = []
                for i in range(rk.stages):
                    ti = t0 if rk.c[i] == 0.0 else (t1 if rk.c[i] == 1.0 else t0 + rk._s(rk.c[i]) * dt)
                    ks.append(rk._f(float(ti), rk._stage(y, ks, rk.a[i][:i], dt)))
                hist.insert(0, ks[0])
                y1 = rk._stage(y, ks, rk.b, dt)
                y = y1 if y1 is not y else [v.clone() for v in y]
            else:
                hist.insert(0, rk._f(float(rk._s(times[k])), y))
                del hist[q:]
                nz = [(hist[j], float(w[k, j])) for j in range(q) if float(w[k, j]) != 0.0]
                out = [torch.empty_like(v) for v in y]
                for i in range(len(y)):
                    self.ops.rk_stage(out[i], y[i], [h[i] for h, _ in nz], [c for _, c in nz])
                y = out
            outs.append(y)
        return outs

    def integrate(self, y0: Sequence[torch.Tensor], t0: float, t_end: float) -> State:
        return self.integrate_times(y0, [t0, t_end])[-1]
