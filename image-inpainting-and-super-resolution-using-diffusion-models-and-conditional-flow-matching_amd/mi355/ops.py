"""Tensor-level wrappers of the single-op C entry points (PyTorch supplies memory and the stream only).

Every function validates its operands on the host (device, dtype, contiguity, shapes) before a
hand-written kernel is launched, enqueues on torch's current HIP stream and never synchronises.
"""
from __future__ import annotations

import collections
import ctypes as C

import torch

from . import _lib
from ._lib import MI355BackendError, check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t: torch.Tensor, name: str, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise MI355BackendError(f"{name} is on {t.device}: the MI355X HIP backend needs device tensors (no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return C.c_void_p(t.data_ptr())


def _same(a, b, na, nb):
    if a.shape != b.shape:
        raise ValueError(f"{na} {tuple(a.shape)} and {nb} {tuple(b.shape)} must have the same shape")


def _opt(t, name, dtype=torch.float32):
    """_req of an operand that may be None."""
    return _req(t, name, dtype) if t is not None else None


# --- marshalling shared by the single-op wrappers (the conv ops, their route queries and the ops that take a workspace) ---
def _host(t, shape=None):
    """A weight or bias the C side reads from host memory -> (its fp32 CPU copy, to be kept alive over the call; a float pointer to it)."""
    if t is None:
        return None, None
    h = t.detach().to("cpu", torch.float32).reshape(shape or t.shape).contiguous()
    return h, C.cast(h.data_ptr(), C.POINTER(C.c_float))


def _conv_out_size(H, W, k, stride=1, resample=0):
    """Output size of a padded k x k conv over an H x W input that is first resampled: 2 nearest x2, 3 a 2x2 average pool."""
    Hc, Wc = (2 * H, 2 * W) if resample == 2 else ((H // 2, W // 2) if resample == 3 else (H, W))
    return (Hc + 2 * (k // 2) - k) // stride + 1, (Wc + 2 * (k // 2) - k) // stride + 1


def _check_emb_res(emb, res, res_mode, B, Co, Ho, Wo):
    if emb is not None and tuple(emb.shape) != (B, Co):
        raise ValueError("emb must be [B, Co]")
    want = (B, Co, Ho, Wo) if res_mode == 1 else (B, Co, Ho // 2, Wo // 2)
    if res is not None and tuple(res.shape) != want:
        raise ValueError(f"res must be {want}")


def _workspace(L, B, channels, hw, device, fill=None):
    """-> (the tensor, to be kept alive over the call; its pointer; its size): mi355_op_workspace_bytes of device memory, every byte `fill` if given."""
    wsb = L.mi355_op_workspace_bytes(B, channels, hw)
    ws = torch.empty(wsb, device=device, dtype=torch.uint8) if fill is None else torch.full((wsb,), int(fill), device=device, dtype=torch.uint8)
    return ws, C.c_void_p(ws.data_ptr()), wsb


def _debug_ptr(debug, or_default):
    """The mi355_debug_config argument; debug None: the default struct (or_default) or NULL - the ops differ in which they hand over."""
    return C.byref(debug) if debug is not None else (C.byref(_lib.debug_config()) if or_default else None)


def _route_dict(route):
    """The words a conv op reports of its launch (the first four, or all eight) -> dict."""
    return dict(zip(("kernel", "form", "tile_m", "tile_n", "reads_nchw", "axpy", "ksplit", "n_mt"), route))


_StepOperands = collections.namedtuple("_StepOperands", "guided B per n stride wf wp keep use_philox seed off")


class Ops:
    """Default op table used by the samplers (tests may inject a recording double with the same methods)."""

    def timestep_embedding(self, t, dim, max_period=10000.0):
        out = torch.empty(t.shape[0], dim, device=t.device, dtype=torch.float32)
        check(_lib.lib().mi355_timestep_embedding(_req(t, "t"), t.shape[0], dim, float(max_period), _req(out, "out"), _stream()))
        return out

    def groupnorm(self, x, gamma, beta, groups=32, eps=1e-5, silu=False):
        B, Cc = x.shape[:2]
        hw = x[0, 0].numel()
        y = torch.empty_like(x)
        check(_lib.lib().mi355_groupnorm(_req(x, "x"), _req(gamma, "gamma"), _req(beta, "beta"), _req(y, "y"), B, Cc, hw, groups,
                                         float(eps), int(silu), _stream()))
        return y

    def euler_step_(self, x, v, dt):
        _same(x, v, "x", "v")
        check(_lib.lib().mi355_euler_step(_req(x, "x"), _req(v, "v"), float(dt), x.numel(), _stream()))
        return x

    def sde_euler_step_(self, x, a, dt, g, b=None, ca=1.0, cb=1.0, dW=None, philox=None, out=None, w=0.0):
        """Euler-Maruyama update in place: x <- x + (ca*a + cb*b) * dt + g * dW (torchsde's Euler step, rounded as its eager expression).
        g: a tensor of x's shape or a float; dW: injected increments, or None with philox = (seed, offset): sqrt(dt) * N(0, 1) from the device
        stream; both None: no noise.  out: a tensor that receives x_old + w * (x_new - x_old) from the same launch.  -> x"""
        _same(x, a, "x", "a")
        if b is not None:
            _same(x, b, "x", "b")
        if isinstance(g, torch.Tensor):
            _same(x, g, "x", "g")
            gp, gs = _req(g, "g"), 0.0
        else:
            gp, gs = None, float(g)
        if dW is not None:
            _same(x, dW, "x", "dW")
        if out is not None:
            _same(x, out, "x", "out")
        seed, off = philox if philox else (0, 0)
        check(_lib.lib().mi355_sde_euler_step(_req(x, "x"), _req(a, "a"), _opt(b, "b"), float(ca), float(cb), float(dt), gp, gs, _opt(dW, "dW"),
                                              int(philox is not None and dW is None), int(seed), int(off), _opt(out, "out"), float(w), x.numel(), _stream()),
              "mi355_sde_euler_step")
        return x

    def ddpm_step_(self, x, eps, z, c_recip, c_recipm1, coef1, coef2, sigma, philox=None):
        """z: injected noise tensor, or None; philox: (seed, offset) for device noise; both None = no noise (i == 0)."""
        _same(x, eps, "x", "eps")
        zp = _opt(z, "z")
        if z is not None:
            _same(x, z, "x", "z")
        seed, off = philox if philox else (0, 0)
        check(_lib.lib().mi355_ddpm_step(_req(x, "x"), _req(eps, "eps"), zp, c_recip, c_recipm1, coef1, coef2, sigma,
                                         int(philox is not None and z is None), seed, off, x.numel(), _stream()))
        return x

    def corrector_step_(self, x, eps, z, c_recip, c_recipm1, rsm1, dt, delta, philox=None):
        _same(x, eps, "x", "eps")
        zp = _opt(z, "z")
        seed, off = philox if philox else (0, 0)
        check(_lib.lib().mi355_corrector_step(_req(x, "x"), _req(eps, "eps"), zp, c_recip, c_recipm1, rsm1, dt, delta,
                                              int(philox is not None and z is None), seed, off, x.numel(), _stream()))
        return x

    def ddim_step_(self, x, eps, c_recip, c_recipm1, acp_prev):
        _same(x, eps, "x", "eps")
        check(_lib.lib().mi355_ddim_step(_req(x, "x"), _req(eps, "eps"), c_recip, c_recipm1, acp_prev, x.numel(), _stream()))
        return x

    def ddim_eta_step_(self, x, eps, z, c_recip, c_recipm1, acp_prev, sigma, philox=None):
        """DDIM(eta) step in place: ddim_step_'s x0 and e2, x <- sqrt(acp_prev) x0 + sqrt(max(1 - acp_prev - sigma^2, 0)) e2 + sigma z.
        z / philox as in ddpm_step_; both None = no noise term (sigma = 0 then gives ddim_step_'s bits)."""
        _same(x, eps, "x", "eps")
        zp = _opt(z, "z")
        if z is not None:
            _same(x, z, "x", "z")
        seed, off = philox if philox else (0, 0)
        check(_lib.lib().mi355_ddim_eta_step(_req(x, "x"), _req(eps, "eps"), zp, c_recip, c_recipm1, acp_prev, float(sigma),
                                             int(philox is not None and z is None), seed, off, x.numel(), _stream()), "mi355_ddim_eta_step")
        return x

    def ddim_eta_cfg_step_(self, x2, eps2, z, w, c_recip, c_recipm1, acp_prev, sigma, philox=None):
        """ddim_eta_step_ on the guided eps, operands as ddpm_cfg_step_."""
        _same(x2, eps2, "x2", "eps2")
        o = self._step_operands(x2, w, philox, z=z, name="x2")
        check(_lib.lib().mi355_ddim_eta_cfg_step(_req(x2, "x2"), _req(eps2, "eps2"), _opt(z, "z"), o.wf, o.wp, o.per, c_recip, c_recipm1, acp_prev,
                                                 float(sigma), o.use_philox, o.seed, o.off, o.n, _stream()), "mi355_ddim_eta_cfg_step")
        return x2

    def dpmpp_step_(self, x, eps, hist, c_recip, c_recipm1, cx, c0, c1):
        """DPM-Solver++ multistep step in place: D = clip(c_recip x - c_recipm1 eps, -1, 1); x <- cx x + c0 D + c1 hist; hist <- D.  hist: the
        previous step's D (not read when c1 == 0), or None (D is not kept; c1 must then be 0).  -> x"""
        _same(x, eps, "x", "eps")
        if hist is not None:
            _same(x, hist, "x", "hist")
        elif float(c1) != 0.0:
            raise ValueError("c1 != 0 needs hist (the previous step's data prediction)")
        check(_lib.lib().mi355_dpmpp_step(_req(x, "x"), _req(eps, "eps"), _opt(hist, "hist"), float(c_recip), float(c_recipm1), float(cx), float(c0), float(c1),
                                          x.numel(), _stream()), "mi355_dpmpp_step")
        return x

    def dpmpp_cfg_step_(self, x2, eps2, hist, w, c_recip, c_recipm1, cx, c0, c1):
        """dpmpp_step_ on the guided eps: x2, eps2, w as in ddim_cfg_step_; hist [B, ...] (or None)."""
        _same(x2, eps2, "x2", "eps2")
        o = self._step_operands(x2, w, hist=hist, name="x2")
        if hist is None and float(c1) != 0.0:
            raise ValueError("c1 != 0 needs hist (the previous step's data prediction)")
        check(_lib.lib().mi355_dpmpp_cfg_step(_req(x2, "x2"), _req(eps2, "eps2"), _opt(hist, "hist"), o.wf, o.wp, o.per, float(c_recip),
                                              float(c_recipm1), float(cx), float(c0), float(c1), o.n, _stream()), "mi355_dpmpp_cfg_step")
        return x2

    def x0_shape_stats(self, x, eps, c_recip, c_recipm1, shaping, w=None, detail=False):
        """The per-image rows of a shaped predictor step (mi355_x0_shape_stats): shape [B, 2] = (f, s), f the guidance-rescale factor of eps and
        s the dynamic threshold of x0 = c_recip x - c_recipm1 (f eps).  x [B, ...]; eps [B, ...], or with w (a float or a [B] tensor) [2B, ...] =
        conditional | unconditional.  shaping: (quantile, max_threshold, rescale_phi), 0 or None = off, or DDPM.x0_shaping.
        detail: also -> [B, 4] = (sigma_c, sigma_g, s_raw, 0).  -> shape, or (shape, detail)"""
        B = x.shape[0]
        guided = w is not None
        if tuple(eps.shape) != ((2 * B if guided else B),) + tuple(x.shape[1:]):
            raise ValueError(f"eps {tuple(eps.shape)} must be x's shape {tuple(x.shape)}" + (" with twice the leading size" if guided else ""))
        o = self._step_operands(x, w, doubled=False)
        sh = _lib.x0_shaping(shaping)
        shape = torch.empty(B, 2, device=x.device, dtype=torch.float32)
        det = torch.empty(B, 4, device=x.device, dtype=torch.float32) if detail else None
        check(_lib.lib().mi355_x0_shape_stats(_req(x, "x"), _req(eps, "eps"), o.wf, o.wp, int(guided), float(c_recip), float(c_recipm1),
                                              C.byref(sh) if sh is not None else None, _req(shape, "shape"), _req(det, "detail") if detail else None,
                                              B, o.per, _stream()), "mi355_x0_shape_stats")
        return (shape, det) if detail else shape

    _STEP_KINDS = {"ddpm": 0, "ddim": 1, "ddim_eta": 2, "dpmpp": 3}

    def x0_shaped_step_(self, kind, x, eps, shape, c_recip, c_recipm1, a, b=0.0, c=0.0, sigma=0.0, z=None, philox=None, hist=None, w=None):
        """One predictor step in place on the rows shape [B, 2] of x0_shape_stats (None: the unshaped step): kind "ddpm" (a, b = coef1, coef2;
        sigma; z / philox as in ddpm_step_), "ddim" (a = acp_prev), "ddim_eta" (a = acp_prev; sigma; z / philox) or "dpmpp" (a, b, c = cx, c0, c1;
        hist).  w (a float or a [B] tensor): the guided form, x and eps [2B, ...] as in ddpm_cfg_step_; z and hist stay [B, ...].  -> x"""
        _same(x, eps, "x", "eps")
        o = self._step_operands(x, w, philox, z=z, hist=hist, shape=shape)
        check(_lib.lib().mi355_x0_shaped_step(self._STEP_KINDS[kind], _req(x, "x"), _req(eps, "eps"), _opt(z, "z"), _opt(hist, "hist"), int(o.guided), o.wf,
                                              o.wp, o.per, float(c_recip), float(c_recipm1), float(a), float(b), float(c), float(sigma), o.use_philox,
                                              o.seed, o.off, _opt(shape, "shape"), o.n, _stream()), "mi355_x0_shaped_step")
        return x

    _STRIDED_KINDS = dict(_STEP_KINDS, corrector=4)

    @staticmethod
    def _wide_out(x, out, guided):
        """Checks of a step on a network output wider than the state: x [B, C, ...] (guided: [2B, C, ...]), out [.., Cw >= C, ...], the same
        leading and trailing sizes -> (B, elements per image of the state, image stride of out)."""
        if guided and x.shape[0] % 2:
            raise ValueError("x holds the state twice: an even leading size")
        if out.dim() != x.dim() or x.dim() < 2 or out.shape[0] != x.shape[0] or out.shape[2:] != x.shape[2:] or out.shape[1] < x.shape[1]:
            raise ValueError(f"the network output {tuple(out.shape)} must be x's shape {tuple(x.shape)} with at least as many channels")
        B = x.shape[0] // 2 if guided else x.shape[0]
        per = x[0].numel() if x.shape[0] else 1
        return B, per, (out[0].numel() if out.shape[0] else per)

    def strided_step_(self, kind, x, out, c_recip, c_recipm1, a, b=0.0, c=0.0, sigma=0.0, z=None, philox=None, hist=None, w=None):
        """x0_shaped_step_'s unshaped steps, and the corrector (kind "corrector": a, b, c = rsm1, dt, delta; never guided), reading eps from the
        first C channels of a wider network output out [B, Cw, ...] in place (mi355_strided_step): nothing is sliced or copied.  -> x"""
        o = self._step_operands(x, w, philox, z=z, hist=hist, out=out)
        check(_lib.lib().mi355_strided_step(self._STRIDED_KINDS[kind], _req(x, "x"), _req(out, "out"), o.stride, _opt(z, "z"), _opt(hist, "hist"),
                                            int(o.guided), o.wf, o.wp, o.per, float(c_recip), float(c_recipm1), float(a), float(b), float(c), float(sigma),
                                            o.use_philox, o.seed, o.off, o.n, _stream()), "mi355_strided_step")
        return x

    def ddpm_lv_step_(self, x, out, z, c_recip, c_recipm1, coef1, coef2, min_log, max_log, philox=None, w=None):
        """The ancestral step of a learned-variance net in place (mi355_ddpm_lv_step): out [B, 2C, ...] is the network output, eps in channels
        [0, C), v in [C, 2C); sigma = exp(0.5 (frac max_log + (1 - frac) min_log)), frac = (v + 1) / 2.  z / philox as in ddpm_step_.  w (a float
        or a [B] tensor): the guided form, x [2B, C, ...] the duplicated state and out [2B, 2C, ...] = conditional | unconditional (v from the
        conditional half); z stays [B, ...].  -> x"""
        o = self._step_operands(x, w, philox, z=z, out=out, twice=True)
        check(_lib.lib().mi355_ddpm_lv_step(_req(x, "x"), _req(out, "out"), _opt(z, "z"), o.wf, o.wp, int(o.guided), o.per, float(c_recip), float(c_recipm1),
                                            float(coef1), float(coef2), float(min_log), float(max_log), o.use_philox, o.seed, o.off, o.B, _stream()),
              "mi355_ddpm_lv_step")
        return x

    _PRED_STEP_KINDS = dict(_STRIDED_KINDS, ddpm_lv=5)

    def pred_step_(self, kind, prediction, x, out, c_recip, c_recipm1, a, b=0.0, c=0.0, sigma=0.0, *, sa=0.0, sb=0.0, min_log=0.0, max_log=0.0, z=None,
                   philox=None, hist=None, w=None, shape=None):
        """One step in place on the raw output `out` of a net of the given prediction ("eps", "x0" or "v"; mi355_pred_step): the data prediction
        is x0_pre of the kind - c_recip x - c_recipm1 out; out itself; sa x - sb out (sa, sb = sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod of
        the step) - and the step goes on from it as x0_shaped_step_ (kind "ddpm", "ddim", "ddim_eta", "dpmpp"; shape: its rows or None),
        strided_step_ (out [B, Cw >= C, ...] read in place; kind "corrector": a, b, c = rsm1, dt, delta) and ddpm_lv_step_ (kind "ddpm_lv": a, b =
        coef1, coef2; min_log, max_log; out [B, 2C, ...]) do.  w: the guided form, x and out [2B, ...].  -> x"""
        o = self._step_operands(x, w, philox, z=z, hist=hist, shape=shape, out=out, twice=kind == "ddpm_lv")
        check(_lib.lib().mi355_pred_step(self._PRED_STEP_KINDS[kind], _lib.prediction_kind(prediction), _req(x, "x"), _req(out, "out"),
                                         0 if o.stride == o.per else o.stride, _opt(z, "z"), _opt(hist, "hist"), int(o.guided), o.wf, o.wp, o.per,
                                         float(c_recip), float(c_recipm1), float(sa), float(sb), float(a), float(b), float(c), float(sigma), float(min_log),
                                         float(max_log), o.use_philox, o.seed, o.off, _opt(shape, "shape"), o.n, _stream()), "mi355_pred_step")
        return x

    def pred_shape_stats(self, prediction, x, out, c_recip, c_recipm1, shaping, *, sa=0.0, sb=0.0, w=None, detail=False):
        """x0_shape_stats on the raw output of a net of the given prediction (mi355_pred_shape_stats): s is the threshold of |x0_pre| of the kind
        (see pred_step_), f the rescale factor of the raw output.  With "x0", x is not read (it only gives the shape).  -> shape, or (shape, detail)"""
        B = x.shape[0]
        guided = w is not None
        if tuple(out.shape) != ((2 * B if guided else B),) + tuple(x.shape[1:]):
            raise ValueError(f"out {tuple(out.shape)} must be x's shape {tuple(x.shape)}" + (" with twice the leading size" if guided else ""))
        o = self._step_operands(x, w, doubled=False)
        sh = _lib.x0_shaping(shaping)
        shape = torch.empty(B, 2, device=x.device, dtype=torch.float32)
        det = torch.empty(B, 4, device=x.device, dtype=torch.float32) if detail else None
        check(_lib.lib().mi355_pred_shape_stats(_lib.prediction_kind(prediction), _req(x, "x"), _req(out, "out"), o.wf, o.wp, int(guided), float(c_recip),
                                                float(c_recipm1), float(sa), float(sb), C.byref(sh) if sh is not None else None, _req(shape, "shape"),
                                                _req(det, "detail") if detail else None, B, o.per, _stream()), "mi355_pred_shape_stats")
        return (shape, det) if detail else shape

    @staticmethod
    def nullspace_op(kind, y_shape=None, pad_value=0.0):
        """The mi355_nullspace_op of a kind ("mask", "block_mean", "bilinear", or its number) for a measurement of shape y_shape [B, C, h_low, w_low]
        (kinds 1, 2) resp. the sentinel pad_value of unknown pixels (kind 0)."""
        k = _lib.NULLSPACE_KINDS.get(kind, kind)
        if k not in (0, 1, 2):
            raise ValueError(f'the null-space operator must be one of {sorted(_lib.NULLSPACE_KINDS)} (or 0..2), got {kind!r}')
        if k == 0:
            return _lib.NullspaceOpC(0, float(pad_value), 0, 0)
        if y_shape is None or len(y_shape) != 4:
            raise ValueError("kinds 1 and 2 need the measurement's shape [B, C, h_low, w_low]")
        return _lib.NullspaceOpC(k, 0.0, int(y_shape[2]), int(y_shape[3]))

    def nullspace_step_(self, op, form, prediction, x, out, y, c_recip, c_recipm1, a, b=0.0, lam=1.0, sigma=0.0, *, sa=0.0, sb=0.0, z=None, philox=None):
        """The null-space (DDNM) predictor step in place, one launch (mi355_nullspace_step): the data prediction x0 of `out` (a net of the given
        prediction; out [B, Cw >= C, H, W] is read in place) is rectified against the measurement y of the operator op (nullspace_op, or a
        NullspaceOpC), x0h = x0 - lam * (A(x0) - y) on the taps of each row, and x [B, C, H, W] moves from x0h: form 0 the ancestral step (a, b = coef1,
        coef2; sigma), form 1 the DDIM(eta) step (a = acp_prev; sigma).  z / philox as in ddpm_step_ (form 1 with neither: no noise term).  -> x"""
        if x.dim() != 4:
            raise ValueError(f"x must be [B, C, H, W], got {tuple(x.shape)}")
        B, per, stride = self._wide_out(x, out, False)
        if z is not None:
            _same(x, z, "x", "z")
        if form not in (0, 1):
            raise ValueError("form must be 0 (ancestral) or 1 (DDIM(eta))")
        want = tuple(x.shape) if op.kind == 0 else (x.shape[0], x.shape[1], op.h_low, op.w_low)
        if tuple(y.shape) != want:
            raise ValueError(f"the measurement y {tuple(y.shape)} must be {want} for this operator")
        seed, off = philox if philox else (0, 0)
        check(_lib.lib().mi355_nullspace_step(C.byref(op), int(form), _lib.prediction_kind(prediction), _req(x, "x"), _req(out, "out"),
                                              0 if stride == per else stride, _req(y, "y"), _opt(z, "z"), x.shape[0], x.shape[1], x.shape[2], x.shape[3],
                                              float(c_recip), float(c_recipm1), float(sa), float(sb), float(a), float(b), float(lam), float(sigma),
                                              int(philox is not None and z is None), int(seed), int(off), _stream()), "mi355_nullspace_step")
        return x

    def block_mean(self, x, size):
        """Average pooling of [..., H, W] planes to size = (h_low, w_low) with window = stride = (H / h_low, W / w_low) (mi355_block_mean): the
        operator A of null-space kind 1, in the step's summation order.  -> [..., h_low, w_low]"""
        if x.dim() < 2:
            raise ValueError("x must have at least two dimensions")
        hl, wl = int(size[0]), int(size[1])
        out = torch.empty(tuple(x.shape[:-2]) + (hl, wl), device=x.device, dtype=torch.float32)
        planes = x.numel() // max(1, x.shape[-2] * x.shape[-1])
        check(_lib.lib().mi355_block_mean(_req(x, "x"), _req(out, "out"), planes, x.shape[-2], x.shape[-1], hl, wl, _stream()), "mi355_block_mean")
        return out

    def q_sample(self, x0, a, b, z=None, philox=None, out=None):
        """The forward marginal q(x_k | x_0) out of place (mi355_q_sample): a x0 + b z with a = sqrt_alphas_cumprod[k], b =
        sqrt_one_minus_alphas_cumprod[k], two rounded products and a sum; z / philox as in ddpm_step_.  x0 is left as it is.  -> out"""
        if z is not None:
            _same(x0, z, "x0", "z")
        out = torch.empty_like(x0) if out is None else out
        _same(x0, out, "x0", "out")
        seed, off = philox if philox else (0, 0)
        check(_lib.lib().mi355_q_sample(_req(out, "out"), _req(x0, "x0"), _opt(z, "z"), float(a), float(b), int(philox is not None and z is None), seed,
                                        off, x0.numel(), _stream()), "mi355_q_sample")
        return out

    def vlb_terms(self, x0, x_k, out, *, c_recip, c_recipm1, coef1, coef2, true_log, model_log=0.0, min_log=0.0, max_log=0.0, k_is_zero, learned,
                  cdf="exact", clip_denoised=True, z=None, philox=None, dst=None, prediction=None, sa=0.0, sb=0.0):
        """One step of the variational bound (mi355_vlb_terms): x0, x_k [B, C, ...], out [B, C or more, ...] the network output (eps in channels
        [0, C); learned: v in [C, 2C), read in place), the step's draw z (or philox = (seed, offset): regenerated) -> float32 [B, 3] = vb (bits/dim:
        the KL of step k > 0, the discretised decoder's NLL with k_is_zero), xstart_mse, mse.  cdf: "exact" (erfc) or "tanh" (guided-diffusion's
        approximation).  dst: a [B, 3] view to write into (its row stride may be wider: a [B, K, 3] tensor's [:, k]).  prediction (None: "eps",
        mi355_vlb_terms itself; "x0", "v": mi355_vlb_terms_pred with sa, sb = sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod of the step):
        x0_hat comes from x0_pre of the kind and mse is taken against the kind's training target (z; x0; sa z - sb x0)."""
        _same(x0, x_k, "x0", "x_k")
        B, per, stride = self._wide_out(x0, out, False)
        if learned and stride < 2 * per:
            raise ValueError(f"a learned-variance net writes twice the state's channels, got {tuple(out.shape)} for the state {tuple(x0.shape)}")
        if z is not None:
            _same(x0, z, "x0", "z")
        if cdf not in ("exact", "tanh"):
            raise ValueError(f'cdf must be "exact" or "tanh", got {cdf!r}')
        if dst is None:
            dst = torch.empty(B, 3, device=x0.device, dtype=torch.float32)
        if not dst.is_cuda or dst.dtype != torch.float32 or dst.shape != (B, 3) or (B and dst.stride(1) != 1):
            raise ValueError("dst must be a float32 device view of shape [B, 3] with unit inner stride")
        seed, off = philox if philox else (0, 0)
        if prediction is not None:
            check(_lib.lib().mi355_vlb_terms_pred(_req(x0, "x0"), _req(x_k, "x_k"), _req(out, "out"), stride, _opt(z, "z"),
                                                  int(philox is not None and z is None), seed, off, float(c_recip), float(c_recipm1), float(coef1),
                                                  float(coef2), float(true_log), float(model_log), float(min_log), float(max_log), int(bool(k_is_zero)),
                                                  int(bool(learned)), int(cdf == "tanh"), int(bool(clip_denoised)), _lib.prediction_kind(prediction),
                                                  float(sa), float(sb), C.c_void_p(dst.data_ptr()), dst.stride(0) if B > 1 else 3, B, per, _stream()),
                  "mi355_vlb_terms_pred")
            return dst
        check(_lib.lib().mi355_vlb_terms(_req(x0, "x0"), _req(x_k, "x_k"), _req(out, "out"), stride, _opt(z, "z"), int(philox is not None and z is None),
                                         seed, off, float(c_recip), float(c_recipm1), float(coef1), float(coef2), float(true_log), float(model_log),
                                         float(min_log), float(max_log), int(bool(k_is_zero)), int(bool(learned)), int(cdf == "tanh"),
                                         int(bool(clip_denoised)), C.c_void_p(dst.data_ptr()), dst.stride(0) if B > 1 else 3, B, per, _stream()),
              "mi355_vlb_terms")
        return dst

    def vlb_prior(self, x0, sqrt_acp_last, sqrt_one_minus_acp_last, terms=None):
        """The prior term of the variational bound (mi355_vlb_prior) -> float32 [B, 2]: column 0 = KL(q(x_K | x0) || N(0, 1)) in bits/dim; with
        terms ([B, K, 3], what vlb_terms wrote for every step) column 1 = the fp64 sum of terms[:, :, 0] and column 0, rounded once."""
        B = x0.shape[0]
        per = x0[0].numel() if B else 1
        K = 0
        if terms is not None:
            if terms.dim() != 3 or terms.shape[0] != B or terms.shape[2] != 3:
                raise ValueError(f"terms must be [B, K, 3], got {tuple(terms.shape)}")
            K = terms.shape[1]
        summary = torch.zeros(B, 2, device=x0.device, dtype=torch.float32)
        check(_lib.lib().mi355_vlb_prior(_req(x0, "x0"), float(sqrt_acp_last), float(sqrt_one_minus_acp_last), _opt(terms, "terms"), 3 * K, K,
                                         _req(summary, "summary"), B, per, _stream()), "mi355_vlb_prior")
        return summary

    def renoise_(self, x, z, a, b, philox=None):
        """The forward move q(x_k | x_{k-1}) in place: x <- a x + b z (a = sqrt(alphas_k), b = sqrt(betas_k)); z / philox as in ddpm_step_."""
        zp = _opt(z, "z")
        if z is not None:
            _same(x, z, "x", "z")
        seed, off = philox if philox else (0, 0)
        check(_lib.lib().mi355_renoise_step(_req(x, "x"), zp, float(a), float(b), int(philox is not None and z is None), seed, off, x.numel(),
                                            _stream()), "mi355_renoise_step")
        return x

    def replace_mask_(self, x, cond, z, pad_value, noisy, sa, sb, philox=None):
        _same(x, cond, "x", "condition")
        zp = _opt(z, "z")
        seed, off = philox if philox else (0, 0)
        check(_lib.lib().mi355_replace_mask(_req(x, "x"), _req(cond, "condition"), zp, float(pad_value), int(noisy), sa, sb,
                                            int(philox is not None and z is None), seed, off, x.numel(), _stream()))
        return x

    # --- tiled sampling (csrc/tile.hip): plan = mi355.engine.tile_plan(image_size, (Hc, Wc), stride, weight) ---
    def tile_gather(self, canvas, image_size, plan):
        """canvas [B, C, Hc, Wc] -> its windows [B * n_windows, C, S, S] in batch order (canvas-major, windows row-major): an exact copy."""
        B, Cc = canvas.shape[:2]
        out = torch.empty(B * plan["n_windows"], Cc, image_size, image_size, device=canvas.device, dtype=torch.float32)
        check(_lib.lib().mi355_tile_gather(_req(canvas, "canvas"), _req(out, "windows"), B, Cc, int(image_size), C.byref(plan["plan"]), _stream()))
        return out

    def tile_labels(self, y, n_windows):
        """labels [B] int32 -> [B * n_windows]: every window of a canvas carries the canvas's label."""
        out = torch.empty(y.shape[0] * int(n_windows), device=y.device, dtype=torch.int32)
        check(_lib.lib().mi355_tile_labels(_req(y, "y", torch.int32), _req(out, "out", torch.int32), y.shape[0], int(n_windows), _stream()))
        return out

    def tile_blend_(self, windows, plan, out=None, x=None, dt=0.0):
        """windows [B * n_windows, C, S, S] -> the per-pixel weighted average on the canvas [B, C, Hc, Wc] (windows in ascending index: num += w v,
        den += w, num / den; mi355_tile_blend), written to out (made if None).  x (None: no update): x <- x + dt * average, in place."""
        S = windows.shape[2]
        if windows.shape[0] % plan["n_windows"]:
            raise ValueError("windows must hold n_windows rows per canvas")
        B, Cc = windows.shape[0] // plan["n_windows"], windows.shape[1]
        shape = (B, Cc, plan["plan"].canvas_h, plan["plan"].canvas_w)
        if out is None:
            out = torch.empty(shape, device=windows.device, dtype=torch.float32)
        if tuple(out.shape) != shape or (x is not None and tuple(x.shape) != shape):
            raise ValueError(f"out and x must be {shape}")
        check(_lib.lib().mi355_tile_blend(_req(windows, "windows"), _req(out, "out"), _opt(x, "x"), float(dt), B, Cc, S, C.byref(plan["plan"]), _stream()))
        return out

    def guidance_seed(self, x, eps, cond, c_recip, c_recipm1, mode, pad_value):
        """-> (g_eps, g_x): cotangent for the U-Net VJP and the direct-path gradient of the per-sample constraint
        (mode 0 = Painting.loss with the pad sentinel masked, 1 = HyperResolution.loss; sampling.py:148-160)."""
        _same(x, eps, "x", "eps")
        _same(x, cond, "x", "condition")
        g_eps, g_x = torch.empty_like(x), torch.empty_like(x)
        check(_lib.lib().mi355_guidance_seed(_req(x, "x"), _req(eps, "eps"), _req(cond, "condition"), float(c_recip), float(c_recipm1),
                                             int(mode), float(pad_value), x[0].numel(), _req(g_eps, "g_eps"), _req(g_x, "g_x"), x.numel(),
                                             _stream()))
        return g_eps, g_x

    def lowres_seed(self, x, eps, y_low, c_recip, c_recipm1):
        """-> (g_eps, g_x, loss): guidance_seed for the low-resolution consistency term, loss[n] = mean((D(x0) - y_low)^2) over sample n with
        D the bilinear reduction to y_low's size (F.interpolate, align_corners=False) and x0 = clip(c_recip x - c_recipm1 eps, -1, 1).  The
        state's height and width must be multiples of y_low's (mi355_lowres_seed)."""
        _same(x, eps, "x", "eps")
        if x.dim() != 4 or y_low.dim() != 4 or tuple(y_low.shape[:2]) != tuple(x.shape[:2]):
            raise ValueError(f"x must be [B, C, H, W] and y_low [B, C, h, w] with the same B and C, got {tuple(x.shape)} and {tuple(y_low.shape)}")
        B, Cc, H, W = x.shape
        hl, wl = y_low.shape[2:]
        g_eps, g_x = torch.empty_like(x), torch.empty_like(x)
        resid = torch.empty_like(y_low)
        loss = torch.empty(B, device=x.device, dtype=torch.float32)
        check(_lib.lib().mi355_lowres_seed(_req(x, "x"), _req(eps, "eps"), _req(y_low, "y_low"), float(c_recip), float(c_recipm1), B, Cc, H, W, hl, wl,
                                           _req(resid, "resid"), _req(g_eps, "g_eps"), _req(g_x, "g_x"), _req(loss, "loss"), _stream()),
              "mi355_lowres_seed")
        return g_eps, g_x, loss

    def guidance_update_(self, x, g_x, vjp, scale, apply):
        """update = -scale * (g_x + vjp); x += update when `apply` (the "before" rule).  -> update"""
        _same(x, g_x, "x", "g_x")
        _same(x, vjp, "x", "vjp")
        upd = torch.empty_like(x)
        check(_lib.lib().mi355_guidance_update(_req(x, "x"), _req(g_x, "g_x"), _req(vjp, "vjp"), float(scale), int(bool(apply)),
                                               _req(upd, "update"), x.numel(), _stream()))
        return upd

    def clip_(self, x, lo=-1.0, hi=1.0):
        check(_lib.lib().mi355_clip(_req(x, "x"), float(lo), float(hi), x.numel(), _stream()))
        return x

    def ema_update_(self, target, source, decay):
        """target = target * decay + source * (1 - decay), in place (cifar10/utils_cifar.py:47-53)."""
        _same(target, source, "target", "source")
        check(_lib.lib().mi355_ema_update(_req(target, "target"), _req(source, "source"), float(decay), float(1 - decay), target.numel(), _stream()))
        return target

    def mse_per_sample(self, a, b):
        """torch.mean((a - b)**2, dim=(1, 2, 3))  (AD/experiments/main.py:299)."""
        _same(a, b, "a", "b")
        out = torch.empty(a.shape[0], device=a.device, dtype=torch.float32)
        check(_lib.lib().mi355_mse_per_sample(_req(a, "a"), _req(b, "b"), _req(out, "out"), a.shape[0], a[0].numel(), _stream()))
        return out

    def image_metrics(self, x, ref, data_range=None, win_size=None, gaussian_weights=False, sigma=1.5, use_sample_covariance=True,
                      K1=0.01, K2=0.03):
        """Per-sample quality of x against ref, both [B, C, H, W] fp32 on the device -> {"mse", "data_range", "psnr", "ssim"}, float32 [B]
        each: skimage's peak_signal_noise_ratio and structural_similarity(channel_axis=0) with their defaults, for the whole batch in one
        launch (calculate_psnr / calculate_ssim and the per-image loop, AD/image_diffusion/trainer2.py:15-30,119-121).  data_range None: each
        sample's max(ref) - min(ref), what the reference passes.  Uniform window: win_size 7; gaussian_weights: radius int(3.5 sigma + 0.5)."""
        for t, name in ((x, "x"), (ref, "ref")):
            if isinstance(t, torch.Tensor) and not t.is_cuda:
                raise MI355BackendError(f"{name} is on {t.device}: the MI355X HIP backend needs device tensors (no CPU fallback)")
        if x.dim() != 4 or x.shape != ref.shape:
            raise MI355BackendError(f"image_metrics: x and ref must be [B, C, H, W] of one shape, got {tuple(x.shape)} and {tuple(ref.shape)}")
        B, Cc, H, W = x.shape
        if data_range is not None and not float(data_range) > 0:
            raise MI355BackendError(f"image_metrics: data_range must be positive (None: each sample's own range), got {data_range}")
        taps = None
        if gaussian_weights:
            # skimage filters with scipy's gaussian_filter(truncate=3.5): radius int(3.5 sigma + 0.5), weights normalised to sum 1
            r = int(3.5 * float(sigma) + 0.5)
            win = 2 * r + 1
            if not 3 <= win <= 15:
                raise MI355BackendError(f"image_metrics: sigma = {sigma} gives a window of {win} taps; 3 to 15 are supported")
            wts = torch.exp(-0.5 * torch.arange(-r, r + 1, dtype=torch.float64) ** 2 / float(sigma) ** 2)
            taps = (C.c_float * win)(*(wts / wts.sum()).float().tolist())
            cov_norm = 1.0
        else:
            win = 7 if win_size is None else int(win_size)
            cov_norm = win * win / (win * win - 1.0) if use_sample_covariance and win > 1 else 1.0
        out = torch.empty(B, 4, device=x.device, dtype=torch.float32)
        check(_lib.lib().mi355_image_metrics(_req(x, "x"), _req(ref, "ref"), _req(out, "out"), B, Cc, H, W,
                                             0.0 if data_range is None else float(data_range), taps, win, cov_norm, float(K1), float(K2), _stream()),
              "mi355_image_metrics")
        return {"mse": out[:, 0], "data_range": out[:, 1], "psnr": out[:, 2], "ssim": out[:, 3]}

    def psnr(self, x, ref, data_range=None):
        """10 log10(R^2 / mse) per sample (image_metrics' "psnr")."""
        return self.image_metrics(x, ref, data_range=data_range)["psnr"]

    def ssim(self, x, ref, **kwargs):
        """Mean structural similarity per sample (image_metrics' "ssim"; the same keywords)."""
        return self.image_metrics(x, ref, **kwargs)["ssim"]

    def lincomb_per_sample(self, x, a, y=None, b=None, out=None):
        """out[n] = a[n] * x[n] (+ b[n] * y[n]) with per-sample fp32 device coefficients a, b of shape [B] (sde_diffusion.py:214-244)."""
        B = x.shape[0]
        if a.shape != (B,) or (b is not None and b.shape != (B,)):
            raise ValueError("per-sample coefficients must have shape [B]")
        if (y is None) != (b is None):
            raise ValueError("y and b go together")
        if y is not None:
            _same(x, y, "x", "y")
        out = torch.empty_like(x) if out is None else out
        check(_lib.lib().mi355_lincomb_per_sample(_req(out, "out"), _req(x, "x"), _opt(y, "y"), _req(a, "a"), _opt(b, "b"), B, x[0].numel(), _stream()))
        return out

    def resize_bilinear(self, x, size):
        """F.interpolate(x, size=size, mode="bilinear", align_corners=False) on an NCHW fp32 device tensor (HIP kernel)."""
        if x.dim() != 4:
            raise ValueError("resize_bilinear expects an NCHW tensor")
        Ho, Wo = int(size[0]), int(size[1])
        out = torch.empty(x.shape[0], x.shape[1], Ho, Wo, device=x.device, dtype=torch.float32)
        check(_lib.lib().mi355_resize_bilinear(_req(x, "x"), _req(out, "out"), x.shape[0] * x.shape[1], x.shape[2], x.shape[3], Ho, Wo,
                                               _stream()), "mi355_resize_bilinear")
        return out

    def paint_patch(self, images, top, left, patch_size, pad_value, outpaint=False):
        """InPainting / OutPainting condition of a whole batch: window (top[n], left[n]) of image n (int32 device tensors [N])."""
        N, Cc, H, W = images.shape
        if tuple(top.shape) != (N,) or tuple(left.shape) != (N,):
            raise ValueError("top / left must have one entry per image")
        out = torch.empty_like(images)
        check(_lib.lib().mi355_paint_patch(_req(images, "images"), _req(top, "top", torch.int32), _req(left, "left", torch.int32),
                                           int(patch_size), float(pad_value), int(bool(outpaint)), _req(out, "out"), N, Cc, H, W, _stream()),
              "mi355_paint_patch")
        return out

    def quantize_u8(self, x):
        out = torch.empty(x.shape, device=x.device, dtype=torch.uint8)
        check(_lib.lib().mi355_quantize_u8(_req(x, "x"), _req(out, "out", torch.uint8), x.numel(), _stream()))
        return out

    def to_unit_range(self, x):
        out = torch.empty_like(x)
        check(_lib.lib().mi355_to_unit_range(_req(x, "x"), _req(out, "out"), x.numel(), _stream()))
        return out

    def randn(self, shape, device, seed, offset=0):
        out = torch.empty(shape, device=device, dtype=torch.float32)
        check(_lib.lib().mi355_randn(_req(out, "out"), int(seed), int(offset), out.numel(), _stream()))
        return out

    # --- adaptive RK45 building blocks (csrc/ode.hip) ---
    def rk_combine(self, out, y0, ks, coeffs):
        """out = y0 + sum_j coeffs[j] * ks[j]  (y0 may be None; coeffs already include dt)."""
        assert len(ks) == len(coeffs) <= 7
        arr = (C.c_float * 7)(*([float(c) for c in coeffs] + [0.0] * (7 - len(coeffs))))
        kp = [_req(k, "k") for k in ks] + [None] * (7 - len(ks))
        check(_lib.lib().mi355_rk_combine(_req(out, "out"), _opt(y0, "y0"), *kp, arr, len(ks), out.numel(), _stream()))
        return out

    def rk_stage(self, out, y0, ks, coeffs, copy_out=None, u8_out=None):
        """One stage of a fixed-step explicit RK method: out = y0 + sum_j coeffs[j] * ks[j] (1 to 4 terms; coeffs already include dt; out may
        be y0: the state updated in place).  The same launch writes the result to copy_out (fp32) and its image bytes, as quantize_u8 of
        the result, to u8_out (uint8)."""
        if not 1 <= len(ks) == len(coeffs) <= 4:
            raise ValueError("rk_stage takes 1 to 4 stage derivatives, one coefficient each")
        _same(out, y0, "out", "y0")
        for k in ks:
            _same(out, k, "out", "k")
        if copy_out is not None:
            _same(out, copy_out, "out", "copy_out")
        if u8_out is not None:
            _same(out, u8_out, "out", "u8_out")
        arr = (C.c_float * 4)(*([float(c) for c in coeffs] + [0.0] * (4 - len(coeffs))))
        kp = (C.c_void_p * 4)(*([_req(k, "k") for k in ks] + [None] * (4 - len(ks))))
        check(_lib.lib().mi355_rk_stage(_req(out, "out"), _req(y0, "y0"), kp, arr, len(ks), out.numel(), _opt(copy_out, "copy_out"),
                                        _opt(u8_out, "u8_out", torch.uint8), _stream()), "mi355_rk_stage")
        return out

    # --- classifier-free guidance (csrc/ode.hip cfg_stage_kernel, csrc/steps.hip) ---
    @staticmethod
    def _cfg_w(w, B):
        """guidance scale -> (host float, device pointer or None, tensor kept alive)."""
        if isinstance(w, torch.Tensor) and w.dim() > 0:
            if tuple(w.shape) != (B,):
                raise ValueError(f"a per-image guidance scale must have shape ({B},), got {tuple(w.shape)}")
            w = w.to(torch.float32).contiguous()
            return 0.0, _req(w, "w"), w
        return float(w), None, None

    def _step_operands(self, x, w, philox=None, *, z=None, hist=None, shape=None, out=None, twice=False, doubled=True, name="x"):
        """What the predictor-step and shape-statistics wrappers hand over besides their tensors and coefficients, with the size checks that go with
        it -> _StepOperands.  w: the guidance scale (a float or a [B] tensor; None: not guided).  doubled: a guided x is [2B, ...] (the step ops;
        the statistics ops keep x [B, ...]).  out: a network output wider than the state (_wide_out; twice: it must hold twice x's channels).  z,
        hist: [B, ...] operands of the B-image state's size; shape: the [B, 2] rows of the statistics; philox: (seed, offset) or None."""
        guided = w is not None
        if out is not None:
            B, per, stride = self._wide_out(x, out, guided)
            if twice and stride != 2 * per:
                raise ValueError(f"a learned-variance net writes twice the state's channels, got {tuple(out.shape)} for the state {tuple(x.shape)}")
        else:
            if guided and doubled and x.shape[0] % 2:
                raise ValueError(f"{name} holds the state twice: an even leading size")
            B = x.shape[0] // 2 if guided and doubled else x.shape[0]
            per = stride = x.numel() // x.shape[0] if x.shape[0] else 1
        n = B * per
        for t, nm in ((z, "z"), (hist, "hist")):
            if t is not None and t.numel() != n:
                raise ValueError(f"{nm} must have the B-image state's size")
        if shape is not None and tuple(shape.shape) != (B, 2):
            raise ValueError(f"shape must be [{B}, 2], got {tuple(shape.shape)}")
        wf, wp, keep = self._cfg_w(w, B) if guided else (0.0, None, None)
        seed, off = philox if philox else (0, 0)
        return _StepOperands(guided, B, per, n, stride, wf, wp, keep, int(philox is not None and z is None), seed, off)

    def cfg_stage(self, out, y0, ks, coeffs, w, dup=False, copy_out=None, u8_out=None):
        """rk_stage over classifier-free-guided derivatives: every ks[j] is [2B, ...] (the conditional evaluation in the first half, the
        unconditional one in the second), g_j = u + w (c - u) with each operation rounded, out = y0 + sum_j coeffs[j] * g_j.  w: a float
        or a [B] tensor.  y0: [B, ...] or None (no base term).  out: [B, ...], or [2B, ...] with dup (the result in both halves).  y0 may be
        out's first half (in place)."""
        if not 1 <= len(ks) == len(coeffs) <= 4:
            raise ValueError("cfg_stage takes 1 to 4 stage derivatives, one coefficient each")
        B2 = ks[0].shape[0]
        if B2 % 2:
            raise ValueError("the derivatives hold the conditional and the unconditional evaluation: an even leading size")
        B = B2 // 2
        half = (B,) + tuple(ks[0].shape[1:])
        for k in ks:
            _same(ks[0], k, "k", "k")
        if tuple(out.shape) != ((B2,) + half[1:] if dup else half):
            raise ValueError(f"out must be {(B2,) + half[1:] if dup else half}, got {tuple(out.shape)}")
        for t, nm in ((y0, "y0"), (copy_out, "copy_out"), (u8_out, "u8_out")):
            if t is not None and tuple(t.shape) != half and not (nm == "y0" and dup and tuple(t.shape) == tuple(out.shape)):
                raise ValueError(f"{nm} must be {half}, got {tuple(t.shape)}")
        n = ks[0].numel() // 2
        wf, wp, keep = self._cfg_w(w, B)
        arr = (C.c_float * 4)(*([float(c) for c in coeffs] + [0.0] * (4 - len(coeffs))))
        kp = (C.c_void_p * 4)(*([_req(k, "k") for k in ks] + [None] * (4 - len(ks))))
        check(_lib.lib().mi355_cfg_stage(_req(out, "out"), _opt(y0, "y0"), kp, arr, len(ks), n, wf, wp, n // B if B else 1, int(bool(dup)),
                                         _opt(copy_out, "copy_out"), _opt(u8_out, "u8_out", torch.uint8), _stream()), "mi355_cfg_stage")
        return out

    def cfg_combine(self, v2, w, out=None):
        """The guided field of one 2B evaluation: v2 [2B, ...] = conditional | unconditional -> u + w (c - u) [B, ...] (cfg_stage, no base term)."""
        if out is None:
            out = torch.empty((v2.shape[0] // 2,) + tuple(v2.shape[1:]), device=v2.device, dtype=torch.float32)
        return self.cfg_stage(out, None, [v2], [1.0], w)

    def ddpm_cfg_step_(self, x2, eps2, z, w, c_recip, c_recipm1, coef1, coef2, sigma, philox=None):
        """ddpm_step_ on the guided eps: x2 [2B, ...] the duplicated state (first half read, both halves written), eps2 [2B, ...] =
        conditional | unconditional; z [B, ...] injected noise or None; philox (seed, offset) indexes the B-image state."""
        _same(x2, eps2, "x2", "eps2")
        o = self._step_operands(x2, w, philox, z=z, name="x2")
        check(_lib.lib().mi355_ddpm_cfg_step(_req(x2, "x2"), _req(eps2, "eps2"), _opt(z, "z"), o.wf, o.wp, o.per, c_recip, c_recipm1, coef1, coef2,
                                             sigma, o.use_philox, o.seed, o.off, o.n, _stream()), "mi355_ddpm_cfg_step")
        return x2

    def ddim_cfg_step_(self, x2, eps2, w, c_recip, c_recipm1, acp_prev):
        """ddim_step_ on the guided eps, operands as ddpm_cfg_step_."""
        _same(x2, eps2, "x2", "eps2")
        o = self._step_operands(x2, w, name="x2")
        check(_lib.lib().mi355_ddim_cfg_step(_req(x2, "x2"), _req(eps2, "eps2"), o.wf, o.wp, o.per, c_recip, c_recipm1, acp_prev, o.n, _stream()),
              "mi355_ddim_cfg_step")
        return x2

    def rk_sqnorm(self, acc, a, sub=None, b=None, b2=None, atol=1.0, rtol=0.0):
        """acc (device fp64 scalar tensor) += sum(((a - sub) / (atol + rtol * max(|b|, |b2|)))**2)."""
        check(_lib.lib().mi355_rk_sqnorm(_req(a, "a"), _opt(sub, "sub"), _opt(b, "b"), _opt(b2, "b2"), float(atol), float(rtol), a.numel(),
                                         _req(acc, "acc", torch.float64), _stream()))
        return acc

    def rk_interp(self, out, y0, y1, ymid, f0, f1, dt, x):
        check(_lib.lib().mi355_rk_interp(_req(out, "out"), _req(y0, "y0"), _req(y1, "y1"), _req(ymid, "ymid"), _req(f0, "f0"), _req(f1, "f1"),
                                         float(dt), float(x), out.numel(), _stream()))
        return out

    # --- parity-test ops on NCHW fp32 tensors (pack -> MFMA kernel -> unpack) ---
    def conv2d(self, x, weight, bias=None, stride=1, resample=0, gn=None, gn_silu=False, dtype=_lib.MI355_F32, x1=None, emb=None,
               res=None, res_mode=1, debug=None, info=None):
        """weight/bias: CPU fp32 tensors in the reference layout [Co,Ci(+Ci1),k,k]; gn = (gamma, beta) device tensors over the
        (concatenated) input channels; x1: second source of a channel concat; emb [B, Co]; res [B, Co, Hr, Wr] with res_mode 1
        (same size) or 2 (nearest x2 of a half-size tensor).  info: a dict that receives what was launched (kernel, form, tile_m, tile_n:
        mi355_conv_extras::route; the call then goes through mi355_conv2d_ex with no fused form asked for, which needs Co % 32 == 0)."""
        B, Cin, H, W = x.shape
        Co, Ci, k, _ = weight.shape
        Cin1 = 0 if x1 is None else x1.shape[1]
        assert Ci == Cin + Cin1
        if x1 is not None and (x1.shape[0] != B or x1.shape[2:] != x.shape[2:]):
            raise ValueError("x1 must match x in batch and spatial size")
        Ho, Wo = _conv_out_size(H, W, k, stride, resample)
        _check_emb_res(emb, res, res_mode, B, Co, Ho, Wo)
        y = torch.empty(B, Co, Ho, Wo, device=x.device, dtype=torch.float32)
        L = _lib.lib()
        ws, wsp, wsb = _workspace(L, B, max(Ci, Co), max(H * W, Ho * Wo), x.device)
        (w, wp), (b, bp) = _host(weight), _host(bias)
        gamma, beta = gn if gn else (None, None)
        args = (_req(x, "x"), _opt(x1, "x1"), Cin1, wp, bp, _req(y, "y"), B, Cin, H, W, Co, k, stride, resample, _opt(gamma, "gamma"),
                _opt(beta, "beta"), int(gn_silu), _opt(emb, "emb"), _opt(res, "res"), int(res_mode), dtype, _debug_ptr(debug, True), wsp, wsb, _stream())
        if info is None:
            check(L.mi355_conv2d(*args), "mi355_conv2d")
        else:
            ex = _lib.ConvExtrasC()
            check(L.mi355_conv2d_ex(*args, C.byref(ex)), "mi355_conv2d_ex")
            info.update(_route_dict(ex.route))
        return y

    def conv2d_ex(self, x, weight, bias, dtype=_lib.MI355_F32, skip=None, sites=(), film=None, debug=None, gn=None, gn_silu=False, emb=None,
                  stats=None):
        """The 3x3 conv of the 8x8 / 4x4 levels with its fused forms (mi355_conv2d_ex): skip = (xs0, xs1 or None, w1 [Co, c0 + c1, 1, 1], b1) is a
        1x1 conv of cat(xs0, xs1) accumulated into the same output; sites = up to two dicts (ctotal, coff, gamma, beta, silu): GroupNorm32 (+SiLU)
        of the output as channels coff.. of a ctotal-channel tensor, written by the epilogue; film [B, 2 Co] on site 0.  Returns
        (y, [act or None per site], skip_done).  gn = (gamma, beta) device tensors: the GroupNorm32 (+ SiLU) input prologue; emb [B, Co]; stats: a
        dict that receives the finalized GroupNorm statistics of the output the launch produced itself (slots, and for slots > 0 a, b [B, Co]
        for gamma = 1, beta = 0: a = rstd, b = -mean rstd of each channel's group) - with gn the 3x3 conv is the warp-specialised kernel's
        prologue form, which carries the skip conv at the large levels."""
        B, Cin, H, W = x.shape
        Co, Ci, k, _ = weight.shape
        assert Ci == Cin and k == 3 and len(sites) <= 2
        y = torch.empty(B, Co, H, W, device=x.device, dtype=torch.float32)
        L = _lib.lib()
        ws, wsp, wsb = _workspace(L, B, max(Ci, Co), H * W, x.device)
        (w, wp), (b, bp) = _host(weight), _host(bias)
        ex = _lib.ConvExtrasC()
        keep = []
        if skip is not None:
            xs0, xs1, w1, b1 = skip
            w1c, b1c = _host(w1, (Co, -1))[0], _host(b1)[0]
            keep += [w1c, b1c]
            ex.skip_x0 = _req(xs0, "skip_x0"); ex.skip_c0 = xs0.shape[1]
            if xs1 is not None:
                ex.skip_x1 = _req(xs1, "skip_x1"); ex.skip_c1 = xs1.shape[1]
            ex.skip_w_host = w1c.data_ptr()
            ex.skip_bias_host = b1c.data_ptr() if b1c is not None else None
        acts = []
        for i, st in enumerate(sites):
            a = torch.full((B, st["ctotal"], H, W), float("nan"), device=x.device, dtype=torch.float32)
            acts.append(a)
            ex.act_out[i] = _req(a, "act_out"); ex.act_gamma[i] = _req(st["gamma"], "gamma"); ex.act_beta[i] = _req(st["beta"], "beta")
            ex.act_ctotal[i] = st["ctotal"]; ex.act_coff[i] = st["coff"]; ex.act_silu[i] = int(st.get("silu", True))
        if film is not None:
            ex.act_film = _req(film, "film")
        if stats is not None:
            one, zero = torch.ones(Co, device=x.device), torch.zeros(Co, device=x.device)
            sa, sb = torch.full((B, Co), float("nan"), device=x.device), torch.full((B, Co), float("nan"), device=x.device)
            keep += [one, zero]
            ex.route[3] = 0x53544154   # MI355_CONV_EXTRAS_STATS: the stat_* fields are present
            ex.stat_gamma = _req(one, "stat_gamma"); ex.stat_beta = _req(zero, "stat_beta"); ex.stat_a = _req(sa, "stat_a"); ex.stat_b = _req(sb, "stat_b")
        _check_emb_res(emb, None, 1, B, Co, H, W)
        gamma, beta = gn if gn else (None, None)
        check(L.mi355_conv2d_ex(_req(x, "x"), None, 0, wp, bp, _req(y, "y"), B, Cin, H, W, Co, 3, 1, 0, _opt(gamma, "gamma"), _opt(beta, "beta"), int(gn_silu),
                                _opt(emb, "emb"), None, 1, dtype, _debug_ptr(debug, True), wsp, wsb, _stream(), C.byref(ex)), "mi355_conv2d_ex")
        if stats is not None:
            stats.update(slots=ex.stat_slots, a=sa if ex.stat_slots > 0 else None, b=sb if ex.stat_slots > 0 else None,
                         kernel=ex.route[0], tile_m=ex.route[2], tile_n=ex.route[3])
        return y, [a if (ex.act_done >> i) & 1 else None for i, a in enumerate(acts)], bool(ex.skip_done)

    def qkv_attention(self, qkv, heads, new_order=False, dtype=_lib.MI355_F32):
        B, width, T = qkv.shape
        ch = width // (3 * heads)
        out = torch.empty(B, heads * ch, T, device=qkv.device, dtype=torch.float32)
        L = _lib.lib()
        ws, wsp, wsb = _workspace(L, B, width, T, qkv.device)
        check(L.mi355_qkv_attention(_req(qkv, "qkv"), _req(out, "out"), B, heads, ch, T, int(new_order), dtype, wsp, wsb, _stream()), "mi355_qkv_attention")
        return out

    def qkv_attention_vjp(self, qkv, grad_out, heads, new_order=False, dtype=_lib.MI355_F32, ws_fill=None):
        """(d qkv_attention / d qkv)^T grad_out through the HIP attention backward (mi355_qkv_attention_vjp): qkv [B, 3 H ch, T],
        grad_out [B, H ch, T] -> grad_qkv [B, 3 H ch, T].  ws_fill: a byte value the workspace is filled with first (tests: 0xFF makes
        every packed intermediate NaN until a kernel writes it)."""
        B, width, T = qkv.shape
        ch = width // (3 * heads)
        if tuple(grad_out.shape) != (B, heads * ch, T):
            raise ValueError(f"grad_out must be {(B, heads * ch, T)}, got {tuple(grad_out.shape)}")
        gq = torch.empty_like(qkv)
        L = _lib.lib()
        ws, wsp, wsb = _workspace(L, B, width, T, qkv.device, ws_fill)
        check(L.mi355_qkv_attention_vjp(_req(qkv, "qkv"), _req(grad_out, "grad_out"), _req(gq, "grad_qkv"), B, heads, ch, T, int(new_order), dtype, wsp, wsb,
                                        _stream()), "mi355_qkv_attention_vjp")
        return gq

    def attn_block_fused(self, x, a, b, weight, bias, heads, new_order=False, dtype=_lib.MI355_F32, debug=None):
        """The fused AttentionBlock front half (mi355_attn_block_fused): attention(qkv(a x + b)) in one kernel.  x [B, C, T]; a, b [B, C] device
        tensors (the per-image, per-channel affine); weight [3C, C] or [3C, C, 1] / bias [3C]: CPU tensors in the reference layout.
        -> (out [B, C, T], form): form = ("image", QB) for the per-(image, head) kernel or ("persistent", NCH, lanes)."""
        B, Cc, T = x.shape
        if tuple(a.shape) != (B, Cc) or tuple(b.shape) != (B, Cc):
            raise ValueError(f"a and b must be {(B, Cc)}")
        (w, wp), (bh, bp) = _host(weight, (weight.shape[0], -1)), _host(bias)
        if tuple(w.shape) != (3 * Cc, Cc) or tuple(bh.shape) != (3 * Cc,):
            raise ValueError(f"weight must be {(3 * Cc, Cc)} and bias {(3 * Cc,)}")
        out = torch.empty(B, Cc, T, device=x.device, dtype=torch.float32)
        L = _lib.lib()
        ws, wsp, wsb = _workspace(L, B, 3 * Cc, T, x.device)
        form = (C.c_int32 * 3)(-1, -1, -1)
        check(L.mi355_attn_block_fused(_req(x, "x"), _req(a, "a"), _req(b, "b"), wp, bp, _req(out, "out"), B, Cc, T, heads, int(new_order), dtype,
                                       _debug_ptr(debug, True), form, wsp, wsb, _stream()), "mi355_attn_block_fused")
        return out, (("image", form[1]) if form[0] == 1 else ("persistent", form[1], form[2]))

    # --- GroupNorm32 test ops: the kernels the network launches, one op each (NCHW fp32 tensors; see include/mi355_sampler.h) ---
    def gn_affine(self, x, gamma, beta, x1=None, film=None, eps=1e-5, dtype=_lib.MI355_F32, apply=None, stats=True):
        """gn_affine_kernel on x [B, C0, *] (and x1 [B, C1, *], the channel concat).  apply: None, "affine" or "silu" (also write y).
        -> dict(a, b [B, C]; mean, rstd [B, 32] if stats; y [B, C, *] if apply; form = NL of the launched template form)."""
        B, C0 = x.shape[:2]
        C1 = 0 if x1 is None else x1.shape[1]
        hw = x[0, 0].numel()
        if x1 is not None and (x1.shape[0] != B or x1[0, 0].numel() != hw):
            raise ValueError("x1 must match x in batch and spatial size")
        Cc = C0 + C1
        if tuple(gamma.shape) != (Cc,) or tuple(beta.shape) != (Cc,) or (film is not None and tuple(film.shape) != (B, 2 * Cc)):
            raise ValueError("gamma / beta must be [C0 + C1], film [B, 2 (C0 + C1)]")
        if apply not in (None, "affine", "silu"):
            raise ValueError("apply must be None, 'affine' or 'silu'")
        dev = x.device
        a = torch.full((B, Cc), float("nan"), device=dev)
        b = torch.full((B, Cc), float("nan"), device=dev)
        mean = torch.full((B, 32), float("nan"), device=dev) if stats else None
        rstd = torch.full((B, 32), float("nan"), device=dev) if stats else None
        y = torch.full((B, Cc) + tuple(x.shape[2:]), float("nan"), device=dev) if apply else None
        form = C.c_int32(-1)
        check(_lib.lib().mi355_gn_affine(_req(x, "x"), _opt(x1, "x1"), _req(gamma, "gamma"), _req(beta, "beta"), _opt(film, "film"), float(eps), _req(a, "a"),
                                         _req(b, "b"), _req(mean, "mean") if stats else None, _req(rstd, "rstd") if stats else None,
                                         _req(y, "y") if apply else None, int(apply == "silu"), C.byref(form), B, C0, C1, hw, dtype, _stream()),
              "mi355_gn_affine")
        return dict(a=a, b=b, mean=mean, rstd=rstd, y=y, form=form.value)

    def conv2d_gn(self, x, weight, bias, gamma, beta, x1=None, weight1=None, bias1=None, film=None, eps=1e-5, stride=1, resample=0,
                  dtype=_lib.MI355_F32, debug=None):
        """One conv (or two: x1, weight1, bias1) with GroupNorm partial sums of the output(s) from the epilogue, then gn_finalize_kernel
        over the channel concat of the outputs.  weight / bias: CPU tensors [Co, Ci, k, k] / [Co].
        -> dict(y, y1, a, b, kernel, slots, form, kernel1, slots1, form1); a / b are NaN when a producer filled no slots."""
        B, Cin, H, W = x.shape
        Co, Ci, k, _ = weight.shape
        assert Ci == Cin
        Co1 = 0
        if x1 is not None:
            Co1, Ci1, k1, _ = weight1.shape
            assert Ci1 == x1.shape[1] and k1 == k and x1.shape[0] == B and x1.shape[2:] == x.shape[2:]
        Ho, Wo = _conv_out_size(H, W, k, stride, 2 if resample == 2 else 0)
        Cc = Co + Co1
        if tuple(gamma.shape) != (Cc,) or tuple(beta.shape) != (Cc,) or (film is not None and tuple(film.shape) != (B, 2 * Cc)):
            raise ValueError("gamma / beta must be [Co + Co1], film [B, 2 (Co + Co1)]")
        dev = x.device
        y = torch.full((B, Co, Ho, Wo), float("nan"), device=dev)
        y1 = torch.full((B, Co1, Ho, Wo), float("nan"), device=dev) if x1 is not None else None
        a = torch.full((B, Cc), float("nan"), device=dev)
        b = torch.full((B, Cc), float("nan"), device=dev)
        (w0, w0p), (b0, b0p), (w1, w1p), (b1, b1p) = _host(weight), _host(bias), _host(weight1), _host(bias1)
        info = (C.c_int32 * 6)()
        check(_lib.lib().mi355_conv2d_gn(_req(x, "x"), w0p, b0p, _req(y, "y"), Cin, Co, _opt(x1, "x1"), w1p, b1p, _opt(y1, "y1"),
                                         x1.shape[1] if x1 is not None else 0, Co1, B, H, W, k, stride, resample, _req(gamma, "gamma"), _req(beta, "beta"),
                                         _opt(film, "film"), float(eps), _req(a, "a"), _req(b, "b"), dtype, _debug_ptr(debug, True), info, _stream()),
              "mi355_conv2d_gn")
        return dict(y=y, y1=y1, a=a, b=b, kernel=info[0], slots=info[1], form=info[2], kernel1=info[3], slots1=info[4], form1=info[5])

    def affine_pool(self, x, a=None, b=None, silu=False, dtype=_lib.MI355_F32):
        """AvgPool2d(2)(silu?(a x + b)) through affine_pool_kernel; a, b [B, C] or both None."""
        B, Cc, H, W = x.shape
        if (a is None) != (b is None) or (a is not None and (tuple(a.shape) != (B, Cc) or tuple(b.shape) != (B, Cc))):
            raise ValueError("a and b must both be [B, C] or both None")
        out = torch.full((B, Cc, H // 2, W // 2), float("nan"), device=x.device)
        check(_lib.lib().mi355_affine_pool(_req(x, "x"), _opt(a, "a"), _opt(b, "b"), int(bool(silu)), _req(out, "out"), B, Cc, H, W, dtype, _stream()),
              "mi355_affine_pool")
        return out

    def gn_silu_vjp(self, x, du, gamma, beta, x1=None, film=None, eps=1e-5, silu=True, du_stride=None, g0=None, g1=None,
                    dtype=_lib.MI355_F32):
        """Data gradient of silu?(GroupNorm32(cat(x, x1)) (1 + scale) + shift) for the cotangent du [B, C0 + C1, *] through
        gn_affine_kernel + gn_silu_bwd_kernel.  g0 / g1: gradients to accumulate into (modified in place), or None: overwritten.
        -> (grad of x, grad of x1 or None)"""
        B, C0 = x.shape[:2]
        C1 = 0 if x1 is None else x1.shape[1]
        hw = x[0, 0].numel()
        Cc = C0 + C1
        if tuple(du.shape[:2]) != (B, Cc) or du[0, 0].numel() != hw:
            raise ValueError("du must be [B, C0 + C1, *] with x's spatial size")
        if tuple(gamma.shape) != (Cc,) or tuple(beta.shape) != (Cc,) or (film is not None and tuple(film.shape) != (B, 2 * Cc)):
            raise ValueError("gamma / beta must be [C0 + C1], film [B, 2 (C0 + C1)]")
        acc0, acc1 = g0 is not None, g1 is not None
        if acc0:
            _same(g0, x, "g0", "x")
        if acc1:
            _same(g1, x1, "g1", "x1")
        g0 = g0 if acc0 else torch.full_like(x, float("nan"))
        g1 = None if x1 is None else (g1 if acc1 else torch.full_like(x1, float("nan")))
        check(_lib.lib().mi355_gn_silu_vjp(_req(x, "x"), _opt(x1, "x1"), _req(gamma, "gamma"), _req(beta, "beta"), _opt(film, "film"), float(eps),
                                           int(bool(silu)), _req(du, "du"), int(du_stride or Cc), _req(g0, "g0"), _opt(g1, "g1"), int(acc0), int(acc1), B, C0,
                                           C1, hw, dtype, _stream()), "mi355_gn_silu_vjp")
        return g0, g1

    def grad_gather(self, src, shape, mode, coff=0, scale=1.0, dst=None, dtype=_lib.MI355_F32):
        """grad_gather_kernel: dst [B, Cd, Hd, Wd] (+)= scale * G(src)[:, coff : coff + Cd]; mode 0 identity, 1 2x2 block sum, 2 src[y/2, x/2],
        3 zero insertion.  shape = (Cd, Hd, Wd); dst: a tensor to accumulate into (in place), or None."""
        B, Cs, Hs, Ws = src.shape
        Cd, Hd, Wd = shape
        acc = dst is not None
        if acc and tuple(dst.shape) != (B, Cd, Hd, Wd):
            raise ValueError("dst must be [B, Cd, Hd, Wd]")
        out = dst if acc else torch.full((B, Cd, Hd, Wd), float("nan"), device=src.device)
        check(_lib.lib().mi355_grad_gather(_req(src, "src"), _req(out, "dst"), B, Cd, Hd, Wd, Hs, Ws, Cs, int(coff), int(mode), int(acc),
                                           float(scale), dtype, _stream()), "mi355_grad_gather")
        return out

    def conv2d_vjp(self, weight, grad_out, c0, c1=0, hw=None, mode=0, g_channels=None, g0=None, g1=None, raw=False, dtype=_lib.MI355_F32,
                   debug=None, ws_fill=None, info=None):
        """The data gradient through one conv as the U-Net backward computes it (mi355_conv2d_vjp: conv_pack_weights_dgrad, then the walker's
        own helper).  weight: CPU tensor [Co, Ci, k, k] of the forward conv cat(x0 [B, c0, h, w], x1 [B, c1, h, w]) -> [B, Co, Ho, Wo], Ci <= c0 + c1;
        grad_out [B, Co, Ho, Wo]; hw = (h, w) of the forward input (None: grad_out's size, mode 0); mode 0 plain, 1 stride 2, 2 nearest x2;
        g_channels: packed channels of grad_out (None: Co rounded up to a chunk).  g0 / g1: gradients to accumulate into (in place), or None:
        overwritten.  raw: return the helper's [B, cin_pad, h, w] buffer (the GroupNorm adjoint's input) instead.  ws_fill: a byte value the
        workspace is filled with first (0xFF: whatever no kernel writes comes back NaN).  info: a dict that receives the conv launch (kernel, form,
        tile_m, tile_n).  -> (grad of x0, grad of x1 or None), or the raw buffer."""
        Co, Ci, k, _ = weight.shape
        B = grad_out.shape[0]
        h, w = hw if hw is not None else tuple(grad_out.shape[2:])
        Ho, Wo = ((h - 1) // 2 + 1, (w - 1) // 2 + 1) if mode == 1 else ((2 * h, 2 * w) if mode == 2 else (h, w))
        if tuple(grad_out.shape) != (B, Co, Ho, Wo):
            raise ValueError(f"grad_out must be {(B, Co, Ho, Wo)}, got {tuple(grad_out.shape)}")
        ch = 16 if dtype == _lib.MI355_F32 else 32
        gch = int(g_channels) if g_channels is not None else (Co + ch - 1) // ch * ch
        cin_pad = (c0 + c1 + 31) // 32 * 32
        dev = grad_out.device
        acc0, acc1 = g0 is not None, g1 is not None
        if raw:
            if acc0 or acc1:
                raise ValueError("raw returns the helper's buffer: there is nothing to accumulate into")
            out = torch.full((B, cin_pad, h, w), float("nan"), device=dev)
        else:
            if (acc0 and tuple(g0.shape) != (B, c0, h, w)) or (acc1 and tuple(g1.shape) != (B, c1, h, w)):
                raise ValueError("g0 / g1 must be [B, c0, h, w] / [B, c1, h, w]")
            g0 = g0 if acc0 else torch.full((B, c0, h, w), float("nan"), device=dev)
            g1 = None if not c1 else (g1 if acc1 else torch.full((B, c1, h, w), float("nan"), device=dev))
        L = _lib.lib()
        ws, wsp, wsb = _workspace(L, B, max(cin_pad, gch), max(h * w, Ho * Wo), dev, ws_fill)
        wh, whp = _host(weight)
        route = (C.c_int32 * 4)(-1, -1, -1, -1)
        check(L.mi355_conv2d_vjp(whp, _req(grad_out, "grad_out"), None if raw else _req(g0, "g0"), _opt(g1, "g1"), _req(out, "du_raw") if raw else None,
                                 int(acc0), int(acc1), B, Co, Ci, int(c0), int(c1), h, w, k, int(mode), gch, dtype, _debug_ptr(debug, False), route, wsp, wsb,
                                 _stream()), "mi355_conv2d_vjp")
        if info is not None:
            info.update(_route_dict(route))
        return out if raw else (g0, g1)

    def conv2d_vjp_route(self, B, Co, Ci, c0, c1, h, w, k, mode=0, dtype=_lib.MI355_F32, debug=None):
        """What conv_route decides for the data-gradient conv of these sizes: host code, nothing is launched (no GPU needed).
        -> dict(kernel, form, tile_m, tile_n)"""
        ch = 16 if dtype == _lib.MI355_F32 else 32
        route = (C.c_int32 * 4)(-1, -1, -1, -1)
        check(_lib.lib().mi355_conv2d_vjp(None, None, None, None, None, 0, 0, B, Co, Ci, int(c0), int(c1), h, w, k, int(mode), (Co + ch - 1) // ch * ch, dtype,
                                          _debug_ptr(debug, False), route, None, 0, None), "mi355_conv2d_vjp")
        return _route_dict(route)

    def conv2d_fwd(self, x, weight, bias=None, stride=1, resample=0, pro=None, pro_silu=False, dtype=_lib.MI355_F32, x1=None, emb=None, res=None,
                   res_mode=1, nchw_src=False, axpy_x=None, axpy_scale=0.0, debug=None, ws_fill=None, info=None):
        """One forward conv as the network launches it (mi355_conv2d_fwd).  weight / bias: CPU tensors [Co, Ci (+ Ci1), k, k] / [Co]; pro = (a, b) device
        tensors [B, Ci + Ci1]: the prologue silu?(a v + b) given directly; x1: second source of a channel concat; emb [B, Co]; res with res_mode 1
        (same size) or 2 (nearest x2 of a half-size tensor); resample 0 or 2.  nchw_src: x (and x1, the condition) are handed over as the first conv's
        NCHW tensors.  axpy_x [B, Co, H, W]: the out conv's Euler update x + axpy_scale v (a copy is updated and returned where the launch applies it).
        ws_fill: a byte value the workspace is filled with first (0xFF: whatever no kernel writes comes back NaN).  info: a dict that receives the
        launch (kernel, form, tile_m, tile_n, reads_nchw, axpy, ksplit, n_mt) and both tensors the op could write: y (NaN before the call) and axpy_x (the copy).  -> y [B, Co, Ho, Wo], or the updated copy of axpy_x."""
        B, Cin, H, W = x.shape
        Co, Ci, k, _ = weight.shape
        Cin1 = 0 if x1 is None else x1.shape[1]
        if Ci != Cin + Cin1:
            raise ValueError(f"weight has {Ci} input channels, the sources {Cin} + {Cin1}")
        if x1 is not None and (x1.shape[0] != B or x1.shape[2:] != x.shape[2:]):
            raise ValueError("x1 must match x in batch and spatial size")
        Ho, Wo = _conv_out_size(H, W, k, stride, 2 if resample == 2 else 0)
        if pro is not None and (tuple(pro[0].shape) != (B, Ci) or tuple(pro[1].shape) != (B, Ci)):
            raise ValueError(f"pro = (a, b) must both be {(B, Ci)}")
        _check_emb_res(emb, res, res_mode, B, Co, Ho, Wo)
        if axpy_x is not None and tuple(axpy_x.shape) != (B, Co, Ho, Wo):
            raise ValueError(f"axpy_x must be {(B, Co, Ho, Wo)}")
        dev = x.device
        y = torch.full((B, Co, Ho, Wo), float("nan"), device=dev)
        xu = axpy_x.clone() if axpy_x is not None else None
        L = _lib.lib()
        ws, wsp, wsb = _workspace(L, B, max(Ci, Co), max(H * W, Ho * Wo), dev, ws_fill)
        (wh, whp), (bh, bhp) = _host(weight), _host(bias)
        pro_a, pro_b = pro if pro else (None, None)
        route = (C.c_int32 * 8)(*([-1] * 8))
        check(L.mi355_conv2d_fwd(_req(x, "x"), _opt(x1, "x1"), Cin1, whp, bhp, _req(y, "y"), B, Cin, H, W, Co, k, int(stride), int(resample),
                                 _opt(pro_a, "pro_a"), _opt(pro_b, "pro_b"), int(bool(pro_silu)), _opt(emb, "emb"), _opt(res, "res"), int(res_mode),
                                 int(bool(nchw_src)), _opt(xu, "axpy_x"), float(axpy_scale), dtype, _debug_ptr(debug, False), route, wsp, wsb, _stream()),
              "mi355_conv2d_fwd")
        if info is not None:
            info.update(_route_dict(route), y=y, axpy_x=xu)
        return xu if route[5] == 1 else y

    def conv2d_fwd_route(self, B, Cin, Co, h, w, k, stride=1, resample=0, Cin1=0, bias=True, pro=False, pro_silu=False, emb=False, res_mode=0,
                         nchw_src=False, axpy=False, dtype=_lib.MI355_F32, debug=None):
        """What conv_route decides for the forward conv conv2d_fwd would launch for these sizes and optional parts (res_mode 0: no residual): host
        code, nothing is launched (no GPU needed).  -> dict(kernel, form, tile_m, tile_n, reads_nchw, axpy, ksplit, n_mt)"""
        some = C.c_void_p(256)   # stands for "present": the route query reads no pointer
        route = (C.c_int32 * 8)(*([-1] * 8))
        check(_lib.lib().mi355_conv2d_fwd(None, None, int(Cin1), None, C.cast(some, C.POINTER(C.c_float)) if bias else None, None, B, Cin, h, w, Co, k,
                                          int(stride), int(resample), some if pro else None, some if pro else None, int(bool(pro_silu)), some if emb else None,
                                          some if res_mode else None, int(res_mode) if res_mode else 1, int(bool(nchw_src)), some if axpy else None, 0.0, dtype,
                                          _debug_ptr(debug, False), route, None, 0, None), "mi355_conv2d_fwd")
        return _route_dict(route)

    # --- the embedding path and the layout kernels, one op each (see include/mi355_sampler.h); these ops synchronise the stream ---
    ELEM = {_lib.MI355_F32: torch.float32, _lib.MI355_BF16: torch.bfloat16, _lib.MI355_BF16X2: torch.bfloat16, _lib.MI355_F16: torch.float16}

    def linear(self, x, wt, bias=None, in_act=False, out_act=False, out=None):
        """out[:B] = silu?(bias + silu?(x) @ wt) through linear_launch.  x [B, K], wt [K, J] (the transposed weight), bias [J] or None; out: a
        tensor [>= B, J] to write into (rows beyond B are not touched), or None.  -> (out, form): form 1 = the K-split small kernel, 0 = the slab kernel."""
        if x.dim() != 2 or wt.dim() != 2 or wt.shape[0] != x.shape[1]:
            raise ValueError(f"x must be [B, K] and wt [K, J], got {tuple(x.shape)} and {tuple(wt.shape)}")
        B, K = x.shape
        J = wt.shape[1]
        if bias is not None and tuple(bias.shape) != (J,):
            raise ValueError(f"bias must be {(J,)}")
        if out is None:
            out = torch.full((B, J), float("nan"), device=x.device)
        elif out.dim() != 2 or out.shape[0] < B or out.shape[1] != J:
            raise ValueError(f"out must be [>= {B}, {J}]")
        form = C.c_int32(-1)
        check(_lib.lib().mi355_linear(_req(x, "x"), _req(wt, "wt"), _opt(bias, "bias"), _req(out, "out"), B, K, J, int(bool(in_act)), int(bool(out_act)),
                                      C.byref(form), _stream()), "mi355_linear")
        return out, form.value

    def label_emb_linear(self, h, lemb, wt, bias, rows, h_div, labels=None, out=None):
        """out[r] = bias + silu(h[r // h_div] + lemb[lab(r)]) @ wt through label_emb_linear_launch, lab(r) = labels[r] or, labels None, r % n_classes.
        h [>= (rows - 1) // h_div + 1, K], lemb [n_classes, K], wt [K, J], bias [J] or None, labels int32 [rows] or None.
        -> (out [rows, J], error word, form): error word 2 = a label out of range (its row gets no label term); form = 16 or 8 rows per slab."""
        if h.dim() != 2 or lemb.dim() != 2 or wt.dim() != 2 or lemb.shape[1] != h.shape[1] or wt.shape[0] != h.shape[1]:
            raise ValueError("h must be [*, K], lemb [n_classes, K] and wt [K, J]")
        K, J, n_classes = h.shape[1], wt.shape[1], lemb.shape[0]
        if rows < 1 or h_div < 1 or h.shape[0] < (rows - 1) // h_div + 1:
            raise ValueError(f"h has {h.shape[0]} rows, rows = {rows} with h_div = {h_div} need {(rows - 1) // max(h_div, 1) + 1}")
        if labels is not None and tuple(labels.shape) != (rows,):
            raise ValueError(f"labels must be {(rows,)}")
        if bias is not None and tuple(bias.shape) != (J,):
            raise ValueError(f"bias must be {(J,)}")
        if out is None:
            out = torch.full((rows, J), float("nan"), device=h.device)
        elif out.dim() != 2 or out.shape[0] < rows or out.shape[1] != J:
            raise ValueError(f"out must be [>= {rows}, {J}]")
        err, form = C.c_int32(-1), C.c_int32(-1)
        check(_lib.lib().mi355_label_emb_linear(_req(h, "h"), int(h_div), _req(lemb, "lemb"), _opt(labels, "labels", torch.int32), n_classes, _req(wt, "wt"),
                                                _opt(bias, "bias"), _req(out, "out"), int(rows), K, J, C.byref(err), C.byref(form), _stream()),
              "mi355_label_emb_linear")
        return out, err.value, form.value

    def emb_gather(self, table, labels, out=None):
        """out[b] = table[labels[b]] through emb_gather_launch; table [n_classes, J], labels int32 [B].  -> (out [B, J], error word)"""
        if table.dim() != 2 or labels.dim() != 1:
            raise ValueError("table must be [n_classes, J] and labels [B]")
        B, J = labels.shape[0], table.shape[1]
        if out is None:
            out = torch.full((B, J), float("nan"), device=table.device)
        elif out.dim() != 2 or out.shape[0] < B or out.shape[1] != J:
            raise ValueError(f"out must be [>= {B}, {J}]")
        err = C.c_int32(-1)
        check(_lib.lib().mi355_emb_gather(_req(table, "table"), _req(labels, "labels", torch.int32), table.shape[0], _req(out, "out"), B, J, C.byref(err),
                                          _stream()), "mi355_emb_gather")
        return out, err.value

    def pack_nhwc(self, x, cond=None, cpad=None, dtype=_lib.MI355_F32):
        """NCHW fp32 x [B, Cx, *] | cond [B, Cc, *] -> NHWC [B, HW, cpad] in the element type of `dtype` (pack_nhwc_launch); cpad None: Cx + Cc rounded
        up to a 16-byte fragment.  The result starts as NaN."""
        B, Cx = x.shape[:2]
        hw = x[0, 0].numel()
        Cc = 0 if cond is None else cond.shape[1]
        if cond is not None and (cond.shape[0] != B or cond[0, 0].numel() != hw):
            raise ValueError("cond must match x in batch and spatial size")
        V = 4 if dtype == _lib.MI355_F32 else 8
        cpad = (Cx + Cc + V - 1) // V * V if cpad is None else int(cpad)
        out = torch.full((B, hw, cpad), float("nan"), device=x.device, dtype=self.ELEM[dtype])
        check(_lib.lib().mi355_pack_nhwc(_req(x, "x"), Cx, _opt(cond, "cond"), Cc, B, hw, cpad, _req(out, "out", self.ELEM[dtype]), dtype, _stream()),
              "mi355_pack_nhwc")
        return out

    def unpack_nchw(self, t, dtype=_lib.MI355_F32):
        """NHWC t [B, HW, C] in the element type of `dtype` -> NCHW fp32 [B, C, HW] (unpack_nchw_launch)."""
        B, hw, Cc = t.shape
        out = torch.full((B, Cc, hw), float("nan"), device=t.device)
        check(_lib.lib().mi355_unpack_nchw(_req(t, "t", self.ELEM[dtype]), B, hw, Cc, _req(out, "out"), dtype, _stream()), "mi355_unpack_nchw")
        return out

    def unpack_channels(self, t, c0, count, dtype=_lib.MI355_F32):
        """Channels c0 .. c0 + count of NHWC t [B, HW, stride] -> NCHW fp32 [B, count, HW] (unpack_channels_launch: fp32 and bf16)."""
        B, hw, stride = t.shape
        if c0 < 0 or count < 1 or c0 + count > stride:
            raise ValueError(f"channels {c0} .. {c0 + count} must lie inside a row of {stride}")
        out = torch.full((B, count, hw), float("nan"), device=t.device)
        check(_lib.lib().mi355_unpack_channels(_req(t, "t", self.ELEM[dtype]), B, hw, stride, int(c0), int(count), _req(out, "out"), dtype, _stream()),
              "mi355_unpack_channels")
        return out

    def resample(self, t, mode, dtype=_lib.MI355_F32):
        """NHWC t [B, H, W, C] in the element type of `dtype`: mode "up" nearest x2 -> [B, 2H, 2W, C]; "pool" AvgPool2d(2) -> [B, H // 2, W // 2, C]
        (resample_launch).  The result starts as NaN."""
        if mode not in ("up", "pool"):
            raise ValueError("mode must be 'up' or 'pool'")
        B, H, W, Cc = t.shape
        Ho, Wo = (2 * H, 2 * W) if mode == "up" else (H // 2, W // 2)
        out = torch.full((B, Ho, Wo, Cc), float("nan"), device=t.device, dtype=self.ELEM[dtype])
        check(_lib.lib().mi355_resample(_req(t, "t", self.ELEM[dtype]), _req(out, "out", self.ELEM[dtype]), B, H, W, Cc, 2 if mode == "up" else 3, dtype,
                                        _stream()), "mi355_resample")
        return out


default_ops = Ops()
