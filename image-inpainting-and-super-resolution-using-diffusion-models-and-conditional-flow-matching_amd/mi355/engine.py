"""UNetEngine: one packed-weight U-Net handle of libmi355_sampler.so plus its workspace.

PyTorch is used for device memory (weight blob, workspace, I/O tensors) and the current stream.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import MI355BackendError, check

_PREC = {"fp32": _lib.MI355_F32, "f32": _lib.MI355_F32, "bf16": _lib.MI355_BF16, "bf16x2": _lib.MI355_BF16X2, "fp16": _lib.MI355_F16, "f16": _lib.MI355_F16}


def param_inventory(cfg: _lib.UNetConfigC):
    """(name, shape) list from the C++ plan builder, reference state_dict order."""
    L = _lib.lib()
    n = check(L.mi355_unet_param_count(C.byref(cfg)), "mi355_unet_param_count")
    out = []
    name = C.create_string_buffer(256)
    shape = (C.c_int64 * 4)()
    nd = C.c_int()
    for i in range(n):
        check(L.mi355_unet_param_info(C.byref(cfg), i, name, 256, shape, C.byref(nd)))
        out.append((name.value.decode(), tuple(int(shape[k]) for k in range(nd.value))))
    return out


def _slices(B: int, mb: int):
    """(lo, hi, whole) for a batch of B run at most mb images at a time; whole: this slice is the caller's batch itself."""
    for lo in range(0, B, mb):
        hi = min(B, lo + mb)
        yield lo, hi, (lo, hi) == (0, B)


def _lab_ptr(lab):
    """The pointer of the int32 labels _labels() made (or a slice of them), or None."""
    return C.c_void_p(lab.data_ptr()) if lab is not None else None


def _host_floats(v, K=None, name=None, per="row of the tables"):
    """Host floats for the library -> (what to pass as const float*, what must stay alive over the call).  K None: a sequence of numbers, as a
    ctypes array (len() gives its length).  K given: a [K] table (tensor, array or list) as a pointer into its CPU fp32 copy; another length is
    the ValueError "`name` must have one entry per `per`"."""
    if K is None:
        arr = (C.c_float * len(v))(*[float(f) for f in v])
        return arr, arr
    t = torch.as_tensor(v, dtype=torch.float32).detach().to("cpu").contiguous()
    if t.numel() != K:
        raise ValueError(f"{name} must have one entry per {per}")
    return C.cast(t.data_ptr(), C.POINTER(C.c_float)), t


def _tableau_arrays(tableau):
    """(a, b, c) -> (stages, ctypes float arrays of a (row-major), b and c)."""
    a, b, c = tableau
    stages = len(b)
    return stages, (C.c_float * (stages * stages))(*[v for row in a for v in row]), (C.c_float * stages)(*b), (C.c_float * stages)(*c)


def feature_cache_args(n_evals, interval=None, branch=None, schedule=None, guidance_scale=None):
    """The feature-cache arguments of a sampler that makes n_evals network evaluations (an int, or a callable that counts them: asked only
    when a cache is given) -> None (no cache: today's code path) or
    (branch k, [full_0, ..., full_{n_evals-1}]).  interval=N is DeepCache's uniform 1:N schedule full[e] = (e % N == 0); schedule is the
    explicit list, one truth value per evaluation in loop order; branch defaults to 1."""
    if interval is None and schedule is None:
        if branch is not None:
            raise ValueError("cache_branch needs a schedule: give cache_interval or cache_schedule")
        return None
    if interval is not None and schedule is not None:
        raise ValueError("cache_interval and cache_schedule both given: a run follows one schedule")
    if guidance_scale is not None:
        raise NotImplementedError("feature caching is not built for the guided (classifier-free guidance) loops yet; nor for the Runge-Kutta / "
                                  "Adams-Bashforth, multistep, shaped, reconstruction and SF2M loops")
    n_evals = n_evals() if callable(n_evals) else n_evals
    k = 1 if branch is None else int(branch)
    if k < 1:
        raise ValueError(f"cache_branch must be >= 1, got {branch}")
    if interval is not None:
        if int(interval) != interval or int(interval) < 1:
            raise ValueError(f"cache_interval must be an integer >= 1, got {interval}")
        full = [e % int(interval) == 0 for e in range(n_evals)]
    else:
        full = [bool(f) for f in schedule]
        if len(full) != n_evals:
            raise ValueError(f"cache_schedule must have one entry per network evaluation ({n_evals}), got {len(full)}")
        if full and not full[0]:
            raise ValueError("cache_schedule[0] must be true: the first evaluation has nothing to reuse")
    return k, full


def ddpm_eval_count(K: int, mode: int, n_corrector: int, walk=None) -> int:
    """The network evaluations of one DDPM run, in loop order: one per downward move and, in the ancestral modes, n_corrector behind each."""
    down = K if walk is None else sum(1 for a, b in zip(walk, list(walk)[1:]) if b < a)
    return down * (1 + (0 if mode == _lib.DDIM else max(0, int(n_corrector))))


def tile_plan(image_size: int, canvas_hw, stride=None, weight="uniform", chunk=None):
    """The window geometry of a tiled call (host only; UNetEngine.tile_plan): asks mi355_tile_count / mi355_tile_origins, so the binding and the
    kernels share one function.  chunk=None leaves the plan's chunk at 1 for the caller to settle."""
    Hc, Wc = (int(v) for v in canvas_hw)
    if stride is None:
        stride = max(1, int(image_size) // 2)
    sy, sx = (int(stride), int(stride)) if isinstance(stride, int) else (int(v) for v in stride)
    if weight not in _lib.TILE_WEIGHTS:
        raise ValueError(f"tiling weight must be one of {sorted(_lib.TILE_WEIGHTS)}, got {weight!r}")
    plan = _lib.TilePlanC(Hc, Wc, sy, sx, _lib.TILE_WEIGHTS[weight], 1 if chunk is None else int(chunk))
    L = _lib.lib()
    cnt = (C.c_int32 * 3)()
    check(L.mi355_tile_count(int(image_size), C.byref(plan), cnt), "mi355_tile_count")
    oy, ox = (C.c_int32 * cnt[0])(), (C.c_int32 * cnt[1])()
    check(L.mi355_tile_origins(int(image_size), C.byref(plan), oy, ox), "mi355_tile_origins")
    oy, ox = list(oy), list(ox)
    return {"plan": plan, "ny": int(cnt[0]), "nx": int(cnt[1]), "n_windows": int(cnt[2]), "oy": oy, "ox": ox,
            "origins": [(a, b) for a in oy for b in ox]}


class UNetEngine:
    def __init__(self, cfg_kwargs: dict, state_dict: Dict[str, torch.Tensor], device, precision: str = "bf16", differentiable: bool = False,
                 debug=None):
        if precision not in _PREC:
            raise ValueError(f"precision must be one of {sorted(_PREC)}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise MI355BackendError(f"UNetEngine needs an MI355X device, got {self.device} (no CPU fallback)")
        self.precision = precision
        self.differentiable = bool(differentiable)
        self.cfg = _lib.make_config(dtype=_PREC[precision], differentiable=differentiable, debug=debug, **cfg_kwargs)
        self.L = _lib.lib()
        inv = param_inventory(self.cfg)
        host = []
        for name, shape in inv:
            if name not in state_dict:
                raise KeyError(f"state_dict is missing {name}")
            t = state_dict[name].detach().to("cpu", torch.float32).contiguous()
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
            host.append(t)
        wbytes = check(self.L.mi355_unet_weight_bytes(C.byref(self.cfg)), "mi355_unet_weight_bytes")
        with torch.cuda.device(self.device):
            self.weights = torch.empty(wbytes, dtype=torch.uint8, device=self.device)
            ptrs = (C.c_void_p * len(host))(*[t.data_ptr() for t in host])
            handle = C.c_void_p()
            check(self.L.mi355_unet_create(C.byref(self.cfg), ptrs, len(host), C.c_void_p(self.weights.data_ptr()), wbytes,
                                           self._stream(), C.byref(handle)), "mi355_unet_create")
        self.handle = handle
        self._ws: Optional[torch.Tensor] = None
        self._ws_bytes: Dict[tuple, int] = {}   # sizes of the samplers' workspaces with tail buffers, per (size function, its arguments)
        self._fwd = None          # (batch, workspace pointer) of the last forward(): what vjp() differentiates
        self._full_state = None   # (batch, workspace pointer) while that workspace holds a full evaluation at that batch: what forward_cached() reuses
        self.in_channels = self.cfg.in_channels
        self.out_channels = self.cfg.out_channels
        self.image_size = self.cfg.image_size
        self.num_classes = int(self.cfg.num_classes)   # 0: no label embedding

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.L.mi355_unet_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # every method that runs the net resets _fwd_state to None; the feature cache's mark goes with it (only forward() / forward_cached() set it again)
    @property
    def _fwd_state(self):
        return self._fwd

    @_fwd_state.setter
    def _fwd_state(self, v):
        self._fwd = v
        if v is None:
            self._full_state = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def check(self, clear: bool = True):
        """Raise MI355BackendError if a launch of this engine gave up a bounded counter wait or met a class label outside
        [0, num_classes) (mi355_unet_status).  Synchronise first to cover the launches already queued; every engine call also checks the flag
        on entry."""
        check(self.L.mi355_unet_status(self.handle, int(clear)), "mi355_unet_status")

    def workspace(self, batch: int):
        need = check(self.L.mi355_unet_workspace_bytes(self.handle, batch), "mi355_unet_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return C.c_void_p(self._ws.data_ptr()), self._ws.numel()

    def _chk(self, t: torch.Tensor, name: str, dtype=torch.float32):
        if not t.is_cuda or t.device != self.device:
            raise MI355BackendError(f"{name} is on {t.device}, the engine lives on {self.device} (no CPU fallback)")
        if t.dtype != dtype or not t.is_contiguous():
            raise TypeError(f"{name} must be contiguous {dtype}")
        return C.c_void_p(t.data_ptr())

    def _ptr(self, t, name: str, dtype=torch.float32):
        """_chk of an operand that may be None."""
        return self._chk(t, name, dtype) if t is not None else None

    @staticmethod
    def _sliced(B: int, mb: int, rows=(), cols=(), outs=(), seed=None):
        """A batch of B run at most mb images at a time: yields per slice (its size, rows, cols, outs, its seed), every operand a tensor or None.
        A slice that is the caller's batch itself gets the caller's own tensors.  rows [B, ...] are cut [lo:hi]: views the call reads and writes
        in place.  cols [n, B, ...] are inputs, cut [:, lo:hi] and made contiguous.  outs [n, B, ...] are outputs: the slice gets a buffer of its
        own, copied into [:, lo:hi] once the caller is done with the slice.  seed: None, or the Philox seed of the batch: the slice draws from
        (seed + slice index) % 2**64."""
        for i, (lo, hi, whole) in enumerate(_slices(B, mb)):
            bufs = [t if whole or t is None else t.new_empty((t.shape[0], hi - lo) + tuple(t.shape[2:])) for t in outs]
            yield (hi - lo, [t if whole or t is None else t[lo:hi] for t in rows],
                   [t if whole or t is None else t[:, lo:hi].contiguous() for t in cols], bufs, None if seed is None else (seed + i) % 2 ** 64)
            for t, buf in zip(outs, bufs):
                if t is not None and not whole:
                    t[:, lo:hi] = buf

    def _labels(self, y, B: int):
        """Class labels -> contiguous int32 [B] on the engine's device (ctypes pointer, tensor kept alive by the caller), or (None, None)."""
        if y is None:
            return None, None
        if not self.num_classes:
            raise ValueError("y (class labels) given to a model built without num_classes")
        if not isinstance(y, torch.Tensor) or y.dtype.is_floating_point or y.dtype.is_complex or y.dtype == torch.bool:
            raise TypeError("y must be an integer tensor of class labels")
        if tuple(y.shape) != (B,):
            raise ValueError(f"y must have shape ({B},), got {tuple(y.shape)}")
        if y.device != self.device:
            raise MI355BackendError(f"y is on {y.device}, the engine lives on {self.device} (no CPU fallback)")
        y = y.to(torch.int32).contiguous()
        return y, C.c_void_p(y.data_ptr())

    def _split(self, x, cond):
        B, Cx, H, W = x.shape
        if H != self.image_size or W != self.image_size:
            raise ValueError(f"expected {self.image_size}x{self.image_size} images, got {H}x{W}")
        Cc = 0
        if cond is not None:
            if cond.shape[0] != B or cond.shape[2:] != x.shape[2:]:
                raise ValueError("condition must match x in batch and spatial size")
            Cc = cond.shape[1]
        if Cx + Cc != self.in_channels:
            raise ValueError(f"x ({Cx}) + condition ({Cc}) channels != in_channels ({self.in_channels})")
        return B, Cx, Cc

    # ---- tiled sampling: canvases larger than the net's frame (MultiDiffusion; mi355_tile_plan in include/mi355_sampler.h) ----
    def tile_plan(self, canvas_hw, stride=None, weight="uniform", chunk=None):
        """The geometry of a tiled call on canvases of canvas_hw = (Hc, Wc), from the library's own host function (mi355_tile_count /
        mi355_tile_origins) -> dict(plan, ny, nx, n_windows, oy, ox, origins).  stride: an int or (sy, sx), default image_size // 2; weight:
        "uniform" or "tent"; chunk: windows per forward (None: as many as a call has, up to max_batch(), decided per call).  origins: the
        (oy, ox) of the windows in batch order (row-major)."""
        return tile_plan(self.image_size, canvas_hw, stride, weight, chunk)

    def _tiled(self, tiling, x, cond, channels: bool = True):
        """The checks of a tiled call -> (B, Cx, Cc, mi355_tile_plan with its chunk settled).  tiling: an object or dict with stride, weight, chunk."""
        get = tiling.get if isinstance(tiling, dict) else lambda k, d=None: getattr(tiling, k, d)
        if x.dim() != 4:
            raise ValueError("x must be [B, C, Hc, Wc]")
        B, Cx, Hc, Wc = x.shape
        Cc = 0
        if cond is not None:
            if cond.shape[0] != B or cond.shape[2:] != x.shape[2:]:
                raise ValueError("condition must match x in batch and spatial size")
            Cc = cond.shape[1]
        if channels and Cx + Cc != self.in_channels:   # (the DDPM loop decides itself what the net sees: the library checks its channels)
            raise ValueError(f"x ({Cx}) + condition ({Cc}) channels != in_channels ({self.in_channels})")
        chunk = get("chunk")
        tp = self.tile_plan((Hc, Wc), get("stride"), get("weight", "uniform") or "uniform", chunk)
        plan = tp["plan"]
        if chunk is None:
            plan.chunk = min(B * tp["n_windows"], self.max_batch())
        elif plan.chunk > self.max_batch():
            raise ValueError(f"tiling chunk ({plan.chunk}) is above max_batch() ({self.max_batch()})")
        return B, Cx, Cc, plan

    def forward_tiled(self, x: torch.Tensor, t: float, cond: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None, *, tiling,
                      out: Optional[torch.Tensor] = None):
        """One tiled evaluation at the host time t (mi355_unet_forward_tiled): x [B, C, Hc, Wc] is cut into overlapping image_size windows, the net
        runs on them in chunks, and the window predictions are blended per pixel -> [B, out_channels, Hc, Wc].  cond: a condition canvas; y: one
        class label per canvas."""
        B, Cx, Cc, plan = self._tiled(tiling, x, cond)
        lab, lab_p = self._labels(y, B)
        if out is None:
            out = torch.empty(B, self.out_channels, x.shape[2], x.shape[3], device=self.device, dtype=torch.float32)
        self._fwd_state = None
        ws, wsb = self._workspace_tiled(B, plan)
        check(self.L.mi355_unet_forward_tiled(self.handle, self._chk(x, "x"), Cx, self._ptr(cond, "condition"), Cc,
                                              float(t), lab_p, self._chk(out, "out"), B, C.byref(plan), ws, wsb, self._stream()),
              "mi355_unet_forward_tiled")
        return out

    def _workspace_tiled(self, B: int, plan):
        need = check(self.L.mi355_tiled_workspace_bytes(self.handle, B, C.byref(plan)), "mi355_tiled_workspace_bytes")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return C.c_void_p(self._ws.data_ptr()), self._ws.numel()

    # ---- classifier-free guidance: v = v_u + w (v_c - v_u), both halves from one evaluation at batch 2B ----
    def _guidance_args(self, guidance_scale, B: int, y, cond, null_label):
        """Host checks of a guided call -> (w float, per-image scale tensor or None, null label int).  guidance_scale: a float or a [B] tensor."""
        if cond is None and y is None:
            raise ValueError("guidance_scale needs something to guide: a condition (cond) and / or class labels (y)")
        nl = 0
        if y is not None:
            if not self.num_classes:
                raise ValueError("y (class labels) given to a model built without num_classes")
            nl = self.num_classes - 1 if null_label is None else int(null_label)   # the usual recipe: K + 1 classes, the last one the null token
            if not 0 <= nl < self.num_classes:
                raise ValueError(f"null_label must be a class index in [0, {self.num_classes}), got {null_label}")
        if isinstance(guidance_scale, torch.Tensor) and guidance_scale.dim() > 0:
            if tuple(guidance_scale.shape) != (B,):
                raise ValueError(f"a per-image guidance_scale must have shape ({B},), got {tuple(guidance_scale.shape)}")
            if guidance_scale.device != self.device:
                raise MI355BackendError(f"guidance_scale is on {guidance_scale.device}, the engine lives on {self.device} (no CPU fallback)")
            return 0.0, guidance_scale.to(torch.float32).contiguous(), nl
        return float(guidance_scale), None, nl

    def cfg_batch(self) -> int:
        """Largest batch of one guided call, max_batch() // 2: every evaluation runs at twice the batch.  An engine whose max_batch() is 1
        cannot run a guided evaluation at all (it is two images) and is refused."""
        mb = self.max_batch()
        if mb < 2:
            raise MI355BackendError(f"guidance evaluates the network at twice the batch, and max_batch() of this engine is {mb}: "
                                    "a guided call needs max_batch() >= 2")
        return mb // 2

    def _workspace_sized(self, name: str, *args):
        """The workspace of a sampler that keeps buffers behind the network's (size function `name`(handle, *args)), its size cached."""
        need = self._ws_bytes.get((name,) + args)
        if need is None:
            need = self._ws_bytes[(name,) + args] = check(getattr(self.L, name)(self.handle, *args), name)
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return C.c_void_p(self._ws.data_ptr()), self._ws.numel()

    def _forward_cfg(self, x, t, cond, out, y, guidance_scale, null_label, none_value):
        """The guided field of one evaluation: the 2B forward, then cfg_stage with no base term."""
        from .ops import default_ops

        B, Cx, Cc = self._split(x, cond)
        lab, _ = self._labels(y, B)
        w, wt, nl = self._guidance_args(guidance_scale, B, lab, cond, null_label)
        mb = self.cfg_batch()
        if out is None:
            out = torch.empty(B, self.out_channels, self.image_size, self.image_size, device=self.device, dtype=torch.float32)
        host_t = isinstance(t, (int, float))
        for _, (xs, cs, ls, ws_, ts, os_), _, _, _ in self._sliced(B, mb, rows=(x, cond, lab, wt, None if host_t else t, out)):
            x2 = torch.cat((xs, xs))
            c2 = torch.cat((cs, torch.full_like(cs, float(none_value)))) if cond is not None else None
            y2 = torch.cat((ls, torch.full_like(ls, nl))) if lab is not None else None
            t2 = t if host_t else torch.cat((ts, ts))
            v2 = self.forward(x2, t2, cond=c2, y=y2)
            default_ops.cfg_combine(v2, w if wt is None else ws_, out=os_)
        self._fwd_state = None
        return out

    def forward(self, x: torch.Tensor, t, cond: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None,
                guidance_scale=None, null_label: Optional[int] = None, none_value: float = -2.0):
        """t: a [B] device tensor, or a host scalar shared by the batch (no device tensor is made for it: mi355_unet_forward_t).
        y: class labels [B] (integer, on the device) of a class-conditional engine: emb = time_embed(.) + label_emb(y)
        (mi355_unet_forward_labels); None = the reference's forward(x, timesteps), which never reads label_emb.
        guidance_scale (a float or a [B] tensor; None: the plain forward): the classifier-free-guided field v_u + w (v_c - v_u) of ONE forward at
        batch 2B, v_u from the none_value-filled condition and / or null_label (default: the last class) - then mi355_cfg_stage."""
        if guidance_scale is not None:
            return self._forward_cfg(x, t, cond, out, y, guidance_scale, null_label, none_value)
        B, Cx, Cc = self._split(x, cond)
        lab, lab_p = self._labels(y, B)
        host_t = isinstance(t, (int, float))
        if not host_t and t.shape != (B,):
            raise ValueError(f"timesteps must have shape ({B},)")
        if out is None:
            out = torch.empty(B, self.out_channels, self.image_size, self.image_size, device=self.device, dtype=torch.float32)
        ws, wsb = self.workspace(B)
        xp, cp = self._chk(x, "x"), self._ptr(cond, "condition")
        tp, op = None if host_t else self._chk(t, "timesteps"), self._chk(out, "out")
        if lab is not None:
            check(self.L.mi355_unet_forward_labels(self.handle, xp, Cx, cp, Cc, tp, float(t) if host_t else 0.0, lab_p, op, B, ws, wsb, self._stream()),
                  "mi355_unet_forward_labels")
        elif host_t:
            check(self.L.mi355_unet_forward_t(self.handle, xp, Cx, cp, Cc, float(t), op, B, ws, wsb, self._stream()), "mi355_unet_forward_t")
        else:
            check(self.L.mi355_unet_forward(self.handle, xp, Cx, cp, Cc, tp, op, B, ws, wsb, self._stream()), "mi355_unet_forward")
        self._fwd_state = self._full_state = (B, self._ws.data_ptr())
        return out

    def cache_branches(self):
        """The feature-cache branches of this net (mi355_unet_cache_info), one dict per branch k = 1..n-1: branch, skip_ops (the plan-op range
        [lo, hi) a shallow evaluation does not issue), tensor (the cached feature's id), shape (C, H, W) and retained_flops (the share of the
        conv + attention FLOPs a shallow evaluation still does).  A schedule with one full evaluation in N costs about
        (1 + (N - 1) * retained_flops) / N of the uncached FLOPs."""
        buf = (C.c_int32 * 8)()
        check(self.L.mi355_unet_cache_info(C.byref(self.cfg), 0, buf), "mi355_unet_cache_info")
        out = []
        for k in range(1, int(buf[0]) + 1):
            check(self.L.mi355_unet_cache_info(C.byref(self.cfg), k, buf), "mi355_unet_cache_info")
            out.append({"branch": k, "skip_ops": (int(buf[1]), int(buf[2])), "tensor": int(buf[3]), "shape": (int(buf[4]), int(buf[5]), int(buf[6])),
                        "retained_flops": buf[7] / 1e6})
        return out

    def forward_cached(self, x: torch.Tensor, t, cond: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
                       y: Optional[torch.Tensor] = None, *, branch: int):
        """forward() under the feature cache (mi355_unet_forward_cached).  branch=0: a full evaluation (as forward()); branch=k: a shallow one,
        which recomputes the k outermost block pairs on this x and t and reuses the feature the last full evaluation left in this engine's
        workspace.  Raises MI355BackendError unless that workspace still holds a full evaluation at this batch (forward() or
        forward_cached(branch=0), with nothing but shallow evaluations since)."""
        B, Cx, Cc = self._split(x, cond)
        lab, lab_p = self._labels(y, B)
        host_t = isinstance(t, (int, float))
        if not host_t and t.shape != (B,):
            raise ValueError(f"timesteps must have shape ({B},)")
        if out is None:
            out = torch.empty(B, self.out_channels, self.image_size, self.image_size, device=self.device, dtype=torch.float32)
        ws, wsb = self.workspace(B)
        state = (B, self._ws.data_ptr())
        if branch and self._full_state != state:
            raise MI355BackendError("forward_cached: this engine's workspace does not hold a full evaluation at this batch (run forward() or "
                                    "forward_cached(branch=0) first; any other call that runs the net, or another batch, discards it)")
        xp, cp = self._chk(x, "x"), self._ptr(cond, "condition")
        tp, op = None if host_t else self._chk(t, "timesteps"), self._chk(out, "out")
        self._fwd_state = None
        check(self.L.mi355_unet_forward_cached(self.handle, xp, Cx, cp, Cc, tp, float(t) if host_t else 0.0, lab_p, op, B, ws, wsb, self._stream(),
                                               int(branch)), "mi355_unet_forward_cached")
        self._full_state = state
        if not branch:
            self._fwd_state = state
        return out

    def vjp(self, grad_out: torch.Tensor, x_channels: Optional[int] = None, out: Optional[torch.Tensor] = None):
        """(d out / d x)^T grad_out of the LAST forward() on this engine (same batch): the reconstruction-guidance gradient
        (AD/image_diffusion/sampling.py:154-163).  Needs an engine built with differentiable=True."""
        if not self.differentiable:
            raise MI355BackendError("vjp needs an engine built with differentiable=True")
        B = grad_out.shape[0]
        Cx = self.out_channels if x_channels is None else int(x_channels)
        if tuple(grad_out.shape) != (B, self.out_channels, self.image_size, self.image_size):
            raise ValueError("grad_out must have the shape of the network output")
        if out is None:
            out = torch.empty(B, Cx, self.image_size, self.image_size, device=self.device, dtype=torch.float32)
        ws, wsb = self.workspace(B)
        if self._fwd_state != (B, self._ws.data_ptr()):
            # the arena offsets scale with the batch and the samplers / profile() reuse the workspace: anything but a forward() of
            # this batch as the last call leaves other activations there, and the gradient would be garbage with rc 0
            raise MI355BackendError("vjp: the last call on this engine was not forward() with the same batch (no activations to differentiate)")
        check(self.L.mi355_unet_vjp(self.handle, self._chk(grad_out, "grad_out"), self._chk(out, "grad_x"), Cx, B, ws, wsb, self._stream()),
              "mi355_unet_vjp")
        return out

    def plan_ops(self):
        """Diagnostics: the plan as a list of dicts (op kinds: 0 GN, 1 conv, 2 attention, 3 resample, 4 pool-affine, 5 fused attention)."""
        names = ("kind", "src0", "src1", "dst", "mode", "ks", "cout", "use_pro", "pro_silu", "res", "res_mode", "gn_site", "heads", "ch", "dst_c", "dst_h")
        buf = (C.c_int32 * 16)()
        out, i = [], 0
        while True:
            n = self.L.mi355_unet_plan_op(self.handle, i, buf)
            if n < 0:
                break
            out.append(dict(zip(names, list(buf))))
            i += 1
            if i >= n:
                break
        return out

    def read_tensor(self, tensor: int, batch: int, shape, gradient: bool = False):
        """Diagnostics: activation (or gradient) `tensor` of the last forward (vjp) as NCHW fp32."""
        out = torch.empty((batch,) + tuple(shape), device=self.device, dtype=torch.float32)
        ws, wsb = self.workspace(batch)
        check(self.L.mi355_unet_read_tensor(self.handle, int(tensor), int(gradient), self._chk(out, "out"), batch, ws, wsb, self._stream()),
              "mi355_unet_read_tensor")
        return out

    def profile(self, x: torch.Tensor, t: torch.Tensor, cond: Optional[torch.Tensor] = None):
        """One forward with HIP events around every op -> list of dicts (kind, ks, cin, cout, h, w, tile, ms, flops, bytes)."""
        B, Cx, Cc = self._split(x, cond)
        out = torch.empty(B, self.out_channels, self.image_size, self.image_size, device=self.device, dtype=torch.float32)
        self._fwd_state = None
        ws, wsb = self.workspace(B)
        cap = 4096
        recs = (_lib.OpProfileC * cap)()
        n = check(self.L.mi355_unet_profile(self.handle, self._chk(x, "x"), Cx, self._ptr(cond, "condition"),
                                            Cc, self._chk(t, "timesteps"), self._chk(out, "out"), B, ws, wsb, self._stream(), recs, cap),
                  "mi355_unet_profile")
        names = {0: "prelude", 1: "gn_stats", 2: "conv", 3: "attention", 4: "resample"}
        return [dict(kind=names[r.kind], ks=r.ks, cin=r.cin, cout=r.cout, h=r.h, w=r.w, tile=(r.tile_m, r.tile_n), ms=r.ms,
                     flops=r.flops, bytes=r.bytes) for r in recs[:min(n, cap)]]

    def stats(self, batch: int):
        s = _lib.UNetStatsC()
        check(self.L.mi355_unet_get_stats(self.handle, batch, C.byref(s)))
        return {"launches": s.launches, "conv_flops": s.conv_flops, "attn_flops": s.attn_flops, "act_bytes": s.act_bytes,
                "weight_bytes": s.weight_bytes}

    def max_batch(self) -> int:
        """Largest batch one call can take: the kernels address every activation tensor through 32-bit buffer offsets, so B x (the largest
        tensor of the plan, per image) must stay under 4 GiB (the library refuses larger launches with "run the batch in slices")."""
        if getattr(self, "max_batch_override", None):
            return int(self.max_batch_override)
        if getattr(self, "_max_batch", None) is None:
            esz = 4 if self.precision in ("fp32", "f32") else 2
            per_image = max([op["dst_c"] * op["dst_h"] * op["dst_h"] * esz for op in self.plan_ops() if op["dst"] >= 0] +
                            [32 * self.image_size * self.image_size * 4])   # the samplers' fp32 scratch holds up to 32 channels
            self._max_batch = max(1, 0xFFFF0000 // (2 * per_image))   # x2: a concat source pair / an in-flight double of the same tensor
        return self._max_batch

    def _traj_u8(self, x: torch.Tensor, n_t: int, keep_traj: bool, want_u8: bool):
        """The samplers' optional outputs for state x over n_t times: (traj [n_t, *x.shape] fp32 or None, u8 image bytes or None)."""
        traj = torch.empty((n_t,) + tuple(x.shape), device=self.device, dtype=torch.float32) if keep_traj else None
        u8 = torch.empty(x.shape, device=self.device, dtype=torch.uint8) if want_u8 else None
        return traj, u8

    def cfm_cfg(self, x: torch.Tensor, t_span: Sequence[float], method="euler", cond: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None,
                guidance_scale=1.0, null_label: Optional[int] = None, none_value: float = -2.0, keep_traj: bool = False, want_u8: bool = False):
        """In-place classifier-free-guided fixed-step integration of x over t_span (mi355_cfm_cfg_sample): the loop of cfm_rk over `method`
        ("euler" is the one-stage tableau) with every evaluation v_u + w (v_c - v_u), run as one forward at batch 2B.  guidance_scale: a float
        or a [B] tensor.  Returns (x, traj or None, u8 or None).  A batch beyond cfg_batch() = max_batch() // 2 runs in slices that
        carry their labels, conditions and scales."""
        from .ode import resolve_tableau

        a, b, c = resolve_tableau(method)
        B, Cx, Cc = self._split(x, cond)
        lab, _ = self._labels(y, B)
        w, wt, nl = self._guidance_args(guidance_scale, B, lab, cond, null_label)
        ts = [float(v) for v in t_span]
        traj, u8 = self._traj_u8(x, len(ts), keep_traj, want_u8)
        for _, (xs, cs, ls, wl, us), _, (tr,), _ in self._sliced(B, self.cfg_batch(), rows=(x, cond, lab, wt, u8), outs=(traj,)):
            self._cfm_cfg_call(xs, ts, (a, b, c), cs, ls, nl, w, wl, float(none_value), tr, us)
        return x, traj, u8

    def _cfm_cfg_call(self, x, ts, tableau, cond, lab, null_label, w, wt, none_value, traj, u8):
        """One mi355_cfm_cfg_sample call (a batch within cfg_batch())."""
        tab = _tableau_arrays(tableau)
        B, Cx, Cc = self._split(x, cond)
        self._fwd_state = None
        ws, wsb = self._workspace_sized("mi355_cfg_workspace_bytes", B, tab[0])
        check(self.L.mi355_cfm_cfg_sample(*self._flow_args(x, Cx, cond, Cc, lab, (none_value, null_label, w, wt)),
                                          *self._fixed_step_args(_host_floats(ts)[0], tab, traj, u8, B, ws, wsb)), "mi355_cfm_cfg_sample")

    def _flow_args(self, x, Cx, cond, Cc, lab, guide=None):
        """What the flow samplers' calls start with: handle, x, Cx, cond, Cc, labels; a guided call (guide = (none_value, null_label, w, per-image
        scales or None)) has none_value before the labels and the rest behind them."""
        head = (self.handle, self._chk(x, "x"), Cx, self._ptr(cond, "condition"), Cc)
        if guide is None:
            return head + (_lab_ptr(lab),)
        none_value, null_label, w, wt = guide
        return head + (none_value, _lab_ptr(lab), int(null_label), float(w), self._ptr(wt, "guidance_scale"))

    def _fixed_step_args(self, arr, tab, traj, u8, B, ws, wsb, ab=()):
        """What the fixed-step samplers' calls end with: the times, [ab: the Adams-Bashforth order and weights,] the tableau (tab: _tableau_arrays),
        the optional outputs, the batch, the workspace and the stream."""
        return (arr, len(arr), *ab, *tab, self._ptr(traj, "traj"), self._ptr(u8, "u8", torch.uint8), B, ws, wsb, self._stream())

    def cfm_euler(self, x: torch.Tensor, t_span: Sequence[float], cond: Optional[torch.Tensor] = None, keep_traj: bool = False,
                  want_u8: bool = False, cond_drift: bool = False, y: Optional[torch.Tensor] = None, guidance_scale=None,
                  null_label: Optional[int] = None, none_value: float = -2.0, cache_interval=None, cache_branch=None, cache_schedule=None,
                  cache_drift: bool = False, tiling=None):
        """In-place Euler integration of x over t_span (host floats).  Returns (x, traj or None, u8 or None).
        tiling (None: every path below, untouched; an object or dict with stride, weight, chunk, e.g. image_diffusion.sampling.Tiling): x (and
        cond) are canvases [B, C, Hc, Wc] with Hc, Wc >= image_size; every step evaluates the net on overlapping windows and blends them
        (mi355_cfm_euler_sample_tiled).  B * windows beyond chunk is handled inside the call.  Not with guidance_scale, cache_* or cond_drift.
        cache_interval / cache_branch / cache_schedule (all None: the paths below, untouched): feature reuse across steps (DeepCache;
        mi355_cfm_euler_sample_cached).  Step k is evaluation k; see mi355.engine.feature_cache_args and cache_branches().  Not with guidance_scale.
        cache_drift=True (needs a schedule; cache_interval=1 measures every step): also returns, as a fourth value, the [n_steps, B] tensor of
        ||F_e - F_prev||^2 / ||F_prev||^2 per image between consecutive full evaluations (-1 in the rows of shallow evaluations and of the first).
        cond_drift: the condition is integrated with derivative `cond` (the concatenated-state sampler of
        mnist/utils_mnist2.py:118-138); the caller's tensor is not modified.
        A batch beyond max_batch() is integrated in slices (every image's trajectory is independent of its batch mates; the kernels chosen for a
        slice may sum in another order than those of the whole batch would).
        y: class labels [B] of a class-conditional engine: every step evaluates model(t_k, x_k, y) (mi355_cfm_euler_sample_labels).
        guidance_scale (a float or a [B] tensor; None: the paths above, untouched): classifier-free guidance, see cfm_cfg."""
        if tiling is not None:
            return self._cfm_euler_tiled(x, t_span, cond, keep_traj, want_u8, y, tiling,
                                         dict(guidance_scale=guidance_scale, cache_interval=cache_interval, cache_branch=cache_branch,
                                              cache_schedule=cache_schedule, cache_drift=cache_drift or None, cond_drift=cond_drift or None))
        cache = feature_cache_args(max(0, len(t_span) - 1), cache_interval, cache_branch, cache_schedule, guidance_scale)
        if cache_drift and cache is None:
            raise ValueError("cache_drift measures the cached feature: give cache_interval or cache_schedule (cache_interval=1: every step)")
        if guidance_scale is not None:
            if cond_drift:
                raise NotImplementedError("cond_drift (the drifting condition of the concatenated-state sampler) is not built with guidance")
            return self.cfm_cfg(x, t_span, "euler", cond, y, guidance_scale, null_label, none_value, keep_traj, want_u8)
        B, Cx, Cc = self._split(x, cond)
        lab, _ = self._labels(y, B)
        arr, _ = _host_floats(t_span)
        traj, u8 = self._traj_u8(x, len(arr), keep_traj, want_u8)
        drift = torch.empty(len(cache[1]), B, device=self.device, dtype=torch.float32) if cache_drift else None
        name = "mi355_cfm_euler_sample" + ("_cached" if cache is not None else "_labels" if lab is not None else "")
        for n, (xs, cs, ls, us), _, (tr, dr), _ in self._sliced(B, self.max_batch(), rows=(x, cond, lab, u8), outs=(traj, drift)):
            self._fwd_state = None
            ws, wsb = self.workspace(n)
            if cache_drift:
                ws, wsb = self._workspace_sized("mi355_feature_cache_workspace_bytes", n, cache[0], 1)
            fc = () if cache is None else (_lib.feature_cache(*cache, drift_ptr=dr.data_ptr() if dr is not None and dr.numel() else None),)
            self._euler_call(name, xs, Cx, cs, Cc, cond_drift, ls, arr, tr, us, n, ws, wsb, *fc)
        return (x, traj, u8, drift) if cache_drift else (x, traj, u8)

    def _euler_call(self, name, x, Cx, cond, Cc, cond_drift, lab, arr, traj, u8, B, ws, wsb, *last):
        """One call of the Euler entry point `name`; all but the plain one take labels, and _cached / _tiled end in their struct (last)."""
        labels = () if name == "mi355_cfm_euler_sample" else (_lab_ptr(lab),)
        check(getattr(self.L, name)(self.handle, self._chk(x, "x"), Cx, self._ptr(cond, "condition"), Cc, int(bool(cond_drift)), *labels, arr, len(arr),
                                    self._ptr(traj, "traj"), self._ptr(u8, "u8", torch.uint8), B, ws, wsb, self._stream(),
                                    *(C.byref(s) for s in last)), name)

    @staticmethod
    def _tiling_refusals(others: dict):
        """tiling together with an option that has no tiled entry point: NotImplementedError naming the pair."""
        for k, v in others.items():
            if v is not None:
                raise NotImplementedError(f"tiling together with {k} is not built (tiled sampling has the plain Euler and DDPM loops only)")

    def _cfm_euler_tiled(self, x, t_span, cond, keep_traj, want_u8, y, tiling, others):
        self._tiling_refusals(others)
        B, Cx, Cc, plan = self._tiled(tiling, x, cond)
        lab, _ = self._labels(y, B)
        arr, _ = _host_floats(t_span)
        traj, u8 = self._traj_u8(x, len(arr), keep_traj, want_u8)
        self._fwd_state = None
        ws, wsb = self._workspace_tiled(B, plan)
        self._euler_call("mi355_cfm_euler_sample_tiled", x, Cx, cond, Cc, False, lab, arr, traj, u8, B, ws, wsb, plan)
        return x, traj, u8

    def _workspace_rk(self, batch: int, stages: int):
        """The sampler workspace with the RK stage buffers behind it (mi355_cfm_rk_workspace_bytes), its size cached per (batch, stages)."""
        return self._workspace_sized("mi355_cfm_rk_workspace_bytes", batch, stages)

    def cfm_rk(self, x: torch.Tensor, t_span: Sequence[float], method="rk4", cond: Optional[torch.Tensor] = None, keep_traj: bool = False,
               want_u8: bool = False, y: Optional[torch.Tensor] = None, cond_drift: bool = False, guidance_scale=None,
               null_label: Optional[int] = None, none_value: float = -2.0):
        """In-place fixed-step explicit Runge-Kutta integration of x over t_span (host floats), one step per interval, the whole loop one
        library call (mi355_cfm_rk_sample).  method: a name of mi355.ode.TABLEAUS ("euler", "midpoint", "heun2", "rk4", "rk4_38") or an
        (a, b, c) tableau of 1 to 4 stages.  Returns (x, traj or None, u8 or None).
        cond: passed to every stage unchanged.  y: class labels [B] of a class-conditional engine.  A batch beyond max_batch() runs in slices,
        as in cfm_euler.  cond_drift, the concatenated-state sampler of cfm_euler, is not built for these methods and is refused (the
        reference runs it with Euler only)."""
        if cond_drift:
            raise NotImplementedError("cond_drift (the drifting condition of the concatenated-state sampler) is built for Euler only: cfm_euler")
        if guidance_scale is not None:   # classifier-free guidance: see cfm_cfg
            return self.cfm_cfg(x, t_span, method, cond, y, guidance_scale, null_label, none_value, keep_traj, want_u8)
        from .ode import resolve_tableau

        tableau = resolve_tableau(method)
        B, Cx, Cc = self._split(x, cond)
        lab, _ = self._labels(y, B)
        arr, _ = _host_floats(t_span)
        traj, u8 = self._traj_u8(x, len(arr), keep_traj, want_u8)
        tab = _tableau_arrays(tableau)
        for n, (xs, cs, ls, us), _, (tr,), _ in self._sliced(B, self.max_batch(), rows=(x, cond, lab, u8), outs=(traj,)):
            self._fwd_state = None
            ws, wsb = self._workspace_rk(n, tab[0])
            check(self.L.mi355_cfm_rk_sample(*self._flow_args(xs, Cx, cs, Cc, ls), *self._fixed_step_args(arr, tab, tr, us, n, ws, wsb)),
                  "mi355_cfm_rk_sample")
        return x, traj, u8

    def cfm_ab(self, x: torch.Tensor, t_span: Sequence[float], method="ab2", cond: Optional[torch.Tensor] = None, keep_traj: bool = False,
               want_u8: bool = False, y: Optional[torch.Tensor] = None, guidance_scale=None, null_label: Optional[int] = None,
               none_value: float = -2.0, start=None):
        """In-place Adams-Bashforth integration of x over t_span (host floats), one step per interval, the whole loop one library call
        (mi355_cfm_ab_sample; with guidance_scale: mi355_cfm_ab_cfg_sample).  method: "ab2", "ab3" or "ab4" (mi355.ode.AB_SOLVERS): one
        evaluation per step from step order - 1 on, the steps before it by the start method (start: a name of mi355.ode.TABLEAUS or an (a, b, c)
        tableau whose c_1 is 0; None: mi355.ode.AB_START[method]).  The weights are mi355.ode.ab_weights(t_span, order).  Returns
        (x, traj or None, u8 or None).  cond, y, guidance_scale, null_label, none_value: as in cfm_rk / cfm_cfg.  A batch beyond max_batch()
        (guided: cfg_batch()) runs in slices."""
        from .ode import AB_SOLVERS, AB_START, ab_weights, resolve_tableau

        if method not in AB_SOLVERS:
            raise NotImplementedError(f"method={method!r}: the Adams-Bashforth samplers are {AB_SOLVERS}")
        order = AB_SOLVERS.index(method) + 2
        tableau = resolve_tableau(AB_START[method] if start is None else start)
        if tableau[2][0] != 0.0:
            raise ValueError("the start method's first stage must sit at t_k (c_1 == 0): it is the history sample")
        B, Cx, Cc = self._split(x, cond)
        lab, _ = self._labels(y, B)
        guided = guidance_scale is not None
        w, wt, nl = self._guidance_args(guidance_scale, B, lab, cond, null_label) if guided else (0.0, None, 0)
        ts = [float(v) for v in t_span]
        weights = ab_weights(ts, order).contiguous()   # CPU fp32 [n_steps, order]
        traj, u8 = self._traj_u8(x, len(ts), keep_traj, want_u8)
        tab = _tableau_arrays(tableau)
        arr, _ = _host_floats(ts)
        wp = C.cast(weights.data_ptr(), C.POINTER(C.c_float)) if weights.numel() else (C.c_float * 1)()
        name = "mi355_cfm_ab_cfg_sample" if guided else "mi355_cfm_ab_sample"
        mb = self.cfg_batch() if guided else self.max_batch()
        for n, (xs, cs, ls, wl, us), _, (tr,), _ in self._sliced(B, mb, rows=(x, cond, lab, wt, u8), outs=(traj,)):
            self._fwd_state = None
            ws, wsb = self._workspace_sized("mi355_cfm_ab_workspace_bytes", n, order, tab[0], int(guided))
            check(getattr(self.L, name)(*self._flow_args(xs, Cx, cs, Cc, ls, (float(none_value), nl, w, wl) if guided else None),
                                        *self._fixed_step_args(arr, tab, tr, us, n, ws, wsb, ab=(order, wp))), name)
        return x, traj, u8

    def cfm_recon(self, x: torch.Tensor, t_span: Sequence[float], y: Optional[torch.Tensor], mode: int, *, scales: Optional[Sequence[float]] = None,
                  replace: Optional[str] = None, final_paste: bool = False, pad_value: float = -2.0, noise: Optional[torch.Tensor] = None,
                  seed: Optional[int] = None, keep_traj: bool = False, want_u8: bool = False, return_loss: bool = False,
                  y_labels: Optional[torch.Tensor] = None):
        """In-place training-free in-painting / super-resolution of x over t_span with this unconditional flow net, the whole loop one library
        call (mi355_cfm_recon_sample): per step an optional paste of the known pixels onto the straight path, the forward, and - where
        scales[k] != 0 - reconstruction guidance through x1_hat = x + (1 - t) v:  x <- x + dt v - dt scales[k] (g_x + vjp).
        y: the measurement; mode 0: a painting condition [B, C, H, W] with pad_value at the unknown pixels, 1: a full-size image
        (HyperResolution.loss), 2: a low-resolution image [B, C, h, w] with H % h == 0 and W % w == 0.
        scales: None (no guidance: any engine) or one float per step (guidance needs differentiable=True).
        replace: None, "coupled" (the known pixels follow the path from this call's own initial state to y) or "fresh" (a new draw per step:
        noise [n_draws, B, C, H, W] injected, or device Philox noise keyed by `seed`; None: drawn from torch's default generator).
        final_paste: one more paste after the last step.  return_loss (mode 2): the per-step, per-sample loss [n_steps, B] (NaN where a step
        was not guided).  y_labels: class labels [B] of a class-conditional engine.
        Returns (x, traj or None, u8 or None, loss or None).  A batch beyond max_batch() runs in slices that carry their rows of y, labels and
        injected draws; with Philox noise each slice draws from its own key (seed + slice index)."""
        B, Cx, _ = self._split(x, None)
        if mode not in (0, 1, 2):
            raise ValueError("mode must be 0 (painting), 1 (hyper-resolution) or 2 (low resolution)")
        rep = {None: 0, "coupled": 1, "fresh": 2}.get(replace, -1)
        if rep < 0:
            raise ValueError(f"replace must be None, 'coupled' or 'fresh', got {replace!r}")
        ts = [float(v) for v in t_span]
        n_steps = len(ts) - 1
        sc = None
        if scales is not None:
            sc = [float(v) for v in scales]
            if len(sc) != n_steps:
                raise ValueError(f"scales must have one entry per step ({n_steps}), got {len(sc)}")
            if any(v != 0.0 for v in sc) and not self.differentiable:
                raise MI355BackendError("cfm_recon: guidance (a non-zero scale) needs an engine built with differentiable=True")
        if return_loss and mode != 2:
            raise ValueError("return_loss is the low-resolution seed's loss (mode 2)")
        hl = wl = 0
        if y is not None:
            want = (B, Cx) if mode == 2 else tuple(x.shape)
            if y.dim() != 4 or tuple(y.shape[:len(want)]) != want:
                raise ValueError(f"y must be {'[B, C, h, w]' if mode == 2 else 'of the shape of x'}, got {tuple(y.shape)}")
            if mode == 2:
                hl, wl = int(y.shape[2]), int(y.shape[3])
        n_draws = n_steps + int(bool(final_paste))
        if noise is not None and (rep != 2 or tuple(noise.shape[1:]) != tuple(x.shape) or noise.shape[0] < n_draws):
            raise ValueError(f"noise is replace='fresh' only and must be [>= {n_draws}, *x.shape], got {tuple(noise.shape)}")
        if rep == 2 and noise is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        lab, _ = self._labels(y_labels, B)
        traj, u8 = self._traj_u8(x, len(ts), keep_traj, want_u8)
        loss = torch.empty(max(n_steps, 0), B, device=self.device, dtype=torch.float32) if return_loss else None
        for _, (xs, ys, ls, us), (nz,), (tr, lo), sd in self._sliced(B, self.max_batch(), rows=(x, y, lab, u8), cols=(noise,), outs=(traj, loss),
                                                                     seed=int(seed or 0)):
            self._cfm_recon_call(xs, ts, ys, int(mode), sc, rep, bool(final_paste), float(pad_value), nz, sd, ls, tr, us, lo, hl, wl)
        return x, traj, u8, loss

    def _cfm_recon_call(self, x, ts, y, mode, scales, rep, final_paste, pad_value, noise, seed, lab, traj, u8, loss, hl, wl):
        """One mi355_cfm_recon_sample call (a batch within max_batch())."""
        B, Cx = x.shape[:2]
        arr, _ = _host_floats(ts)
        sarr = (C.c_float * max(1, len(ts) - 1))(*scales) if scales is not None else None
        self._fwd_state = None
        ws, wsb = self._workspace_sized("mi355_cfm_recon_workspace_bytes", B, hl, wl)
        check(self.L.mi355_cfm_recon_sample(self.handle, self._chk(x, "x"), Cx, _lab_ptr(lab), arr, len(ts), self._ptr(y, "y"), mode, pad_value, hl, wl,
                                            sarr, rep, int(final_paste), self._ptr(noise, "noise"), seed, self._ptr(traj, "traj"),
                                            self._ptr(u8, "u8", torch.uint8), self._ptr(loss, "loss"), B, ws, wsb, self._stream()),
              "mi355_cfm_recon_sample")

    def sf2m_euler(self, score_engine: "UNetEngine", x: torch.Tensor, t_grid: Sequence[float], sigma: float, reverse: bool = False,
                   y: Optional[torch.Tensor] = None, dW: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                   outputs: Optional[Sequence[Tuple[int, float]]] = None):
        """In-place SF2M Euler-Maruyama integration of x over the step grid t_grid (host floats, fp32 boundaries), this engine as the flow
        `model`, score_engine as `score_model` (mi355_sf2m_euler_sample):  x <- x + (model(t, x) + score_model(t, x)) * dt + sigma * dW,
        reverse: both nets at 1 - t and -model + score_model.
        y: class labels [B] used by both nets.  dW: injected increments [n_steps, B, C, H, W]; None: device Philox noise keyed by `seed`
        (None: drawn from torch's default generator).  outputs: (step k, weight w) pairs -> returns traj [len(outputs), B, C, H, W] with
        traj[j] = x_k + w * (x_{k+1} - x_k), or None.  Returns (x, traj).
        A batch beyond min(max_batch()) of the two engines runs in slices; with Philox noise each slice draws from its own key (seed + slice)."""
        if not isinstance(score_engine, UNetEngine) or score_engine.device != self.device:
            raise MI355BackendError("sf2m_euler: score_engine must be a UNetEngine on the same device")
        B, Cx, _ = self._split(x, None)
        ts = [float(v) for v in t_grid]
        n = len(ts) - 1
        if n < 1:
            raise ValueError("sf2m_euler: t_grid needs at least two times (one step)")
        outs = [(int(k), float(w)) for k, w in (outputs or [])]
        if dW is not None and tuple(dW.shape) != (n,) + tuple(x.shape):
            raise ValueError(f"dW must be [n_steps, *x.shape] = {(n,) + tuple(x.shape)}, got {tuple(dW.shape)}")
        if dW is None and seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        lab_eng = self if self.num_classes else score_engine   # the net without num_classes is refused by the library (both must be conditional)
        lab, _ = lab_eng._labels(y, B)
        mb = min(self.max_batch(), score_engine.max_batch())
        traj = self._traj_u8(x, len(outs), bool(outs), False)[0]
        grid, _ = _host_floats(ts)
        osteps = (C.c_int32 * max(1, len(outs)))(*[k for k, _ in outs])
        ows = (C.c_float * max(1, len(outs)))(*[w for _, w in outs])
        for nb, (xs, ls), (dw,), (tr,), sd in self._sliced(B, mb, rows=(x, lab), cols=(dW,), outs=(traj,), seed=seed if dW is None else None):
            self._fwd_state = None
            score_engine._fwd_state = None
            ws_d, wsb_d = self.workspace(nb)
            ws_s, wsb_s = score_engine.workspace(nb)
            check(self.L.mi355_sf2m_euler_sample(self.handle, score_engine.handle, self._chk(xs, "x"), Cx, _lab_ptr(ls), grid, n, float(sigma),
                                                 int(bool(reverse)), self._ptr(dw, "dW"), int(sd or 0) % 2 ** 64, osteps, ows, len(outs),
                                                 self._ptr(tr, "traj"), nb, ws_d, wsb_d, ws_s, wsb_s, self._stream()), "mi355_sf2m_euler_sample")
        return x, traj

    def ddpm_sample(self, x: torch.Tensor, tables: Dict[str, torch.Tensor], *, mode: int, cond: Optional[torch.Tensor] = None,
                    noise: Optional[torch.Tensor] = None, n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0, start_fraction=1.0,
                    noise_condition=True, pad_value=-2.0, none_value=-2.0, seed=0, guidance_scale=None, cache_interval=None, cache_branch=None,
                    cache_schedule=None, tiling=None, prediction=None, y: Optional[torch.Tensor] = None, null_label: Optional[int] = None,
                    timesteps=None, train_steps=None, ddim_sigma=None, walk=None):
        """In-place reverse-denoising loop.  tables: name -> CPU fp32 tensor [Ns] (DDPM buffers).
        prediction (None or "eps": every path below, untouched; "x0", "v"): what the net's output stands for; such a call runs through ddpm_pred
        (mi355_ddpm_pred_sample).  Not with tiling or cache_*.
        tiling (None: every path below, untouched; an object or dict with stride, weight, chunk): x, cond and the injected noise are canvases
        [.., C, Hc, Wc] with Hc, Wc >= image_size; every evaluation runs the net on overlapping windows and blends the eps predictions, the step
        arithmetic is the loop's own on the canvas (mi355_ddpm_sample_tiled).  Not with guidance_scale or cache_*.
        cache_interval / cache_branch / cache_schedule (all None: the paths below, untouched): feature reuse across evaluations (DeepCache;
        mi355_ddpm_sample_sched_cached; an unscheduled call runs as the identity schedule, which is bit-identical).  Evaluations are numbered in loop
        order, correctors included (ddpm_eval_count); see mi355.engine.feature_cache_args and cache_branches().  Not with guidance_scale.
        timesteps / train_steps (both or neither; None: exactly the unscheduled calls): `tables` are the K respaced tables of a RespacedDDPM, step k
        sits at training index timesteps[k] of train_steps (mi355_ddpm_sample_sched / mi355_ddpm_cfg_sample_sched).  With them, ddim_sigma ([K] floats,
        DDIM mode: the DDIM(eta) step) and walk (levels K, ..., 0 moving by +-1, e.g. conditioning.repaint_walk; upward moves re-noise with
        sqrt(alphas), sqrt(betas) of `tables`) may be given.
        guidance_scale (a float or a [B] tensor; None: mi355_ddpm_sample, untouched): classifier-free guidance of the predictor's eps
        (mi355_ddpm_cfg_sample; Amortized mode, or DDIM with a condition, on a 2C-input net), eps_u from the none_value-filled condition and, with
        y (class labels [B]), null_label (default: the last class).  A batch beyond cfg_batch() runs in slices (Philox: seed + slice index)."""
        B = x.shape[0]
        if _lib.prediction_kind(prediction) != 0:
            for what, v in (("tiling", tiling), ("cache_interval", cache_interval), ("cache_branch", cache_branch), ("cache_schedule", cache_schedule)):
                if v is not None:
                    raise NotImplementedError(f"{what} is not built for an x0- or v-prediction net (prediction={prediction!r})")
            return self.ddpm_pred(x, tables, prediction, mode=mode, cond=cond, noise=noise, n_corrector=n_corrector, delta=delta, tmin=tmin, tmax=tmax,
                                  start_fraction=start_fraction, noise_condition=noise_condition, pad_value=pad_value, none_value=none_value, seed=seed,
                                  guidance_scale=guidance_scale, y=y, null_label=null_label, timesteps=timesteps, train_steps=train_steps,
                                  ddim_sigma=ddim_sigma, walk=walk)
        if cond is not None and cond.shape != x.shape:
            raise ValueError("condition must have the shape of x")
        if guidance_scale is None and y is not None:
            raise NotImplementedError("ddpm_sample takes class labels on the guided path only (guidance_scale=)")
        if tiling is not None:
            self._tiling_refusals(dict(guidance_scale=guidance_scale, cache_interval=cache_interval, cache_branch=cache_branch,
                                       cache_schedule=cache_schedule))
        sched = self._ddpm_schedule(tables, timesteps, train_steps, ddim_sigma, walk)
        cache = feature_cache_args(lambda: ddpm_eval_count(int(tables["alphas_cumprod_prev"].numel()), mode, n_corrector, walk), cache_interval,
                                   cache_branch, cache_schedule, guidance_scale)
        if cache is not None and sched is None:   # the cached loop is the scheduled one: steps 0..K-1 of K is the unscheduled loop bit for bit
            K = int(tables["alphas_cumprod_prev"].numel())
            sched = self._ddpm_schedule(tables, list(range(K)), K, None, None)
        if noise is not None and noise.shape[1:] != x.shape:
            raise ValueError("injected noise must be [n_draws, B, C, H, W]")
        if guidance_scale is not None:
            if mode not in (_lib.DDPM_AMORTIZED, _lib.DDIM):
                raise NotImplementedError("guidance is built for the amortized sampler and for DDIM with a condition (prior and replacement are refused)")
            lab, _ = self._labels(y, B)
            w, wt, nl = self._guidance_args(guidance_scale, B, lab, cond, null_label)
            for _, (xs, cn, ls, wl), (nz,), _, sd in self._sliced(B, self.cfg_batch(), rows=(x, cond, lab, wt), cols=(noise,), seed=seed):
                self._ddpm_cfg_call(xs, tables, mode, cn, ls, nl, w, wl, nz,
                                    dict(n_corrector=n_corrector, delta=delta, tmin=tmin, tmax=tmax, none_value=none_value, seed=sd),
                                    **({} if sched is None else {"sched": sched}))
            return x
        tb, keep = self._ddpm_tables(tables)
        self._fwd_state = None
        opt = self._ddpm_options(mode, cond, seed, none_value, n_corrector, delta, tmin, tmax, start_fraction, noise_condition, pad_value)
        if tiling is not None:
            plan = self._tiled(tiling, x, None, channels=False)[3]
            ws, wsb = self._workspace_tiled(B, plan)
            name, mid, last = "mi355_ddpm_sample_tiled", (None if sched is None else sched[0],), (plan,)
        else:
            name = "mi355_ddpm_sample" if sched is None else "mi355_ddpm_sample_sched" if cache is None else "mi355_ddpm_sample_sched_cached"
            ws, wsb = self.workspace(B)
            mid, last = () if sched is None else (sched[0],), () if cache is None else (_lib.feature_cache(*cache),)
        self._ddpm_call(name, x, cond, tb, opt, B, ws, wsb, mid=mid, noise=self._noise_args(noise), last=last)
        del keep
        return x

    def ddpm_multistep(self, x: torch.Tensor, tables: Dict[str, torch.Tensor], coefs, *, cond: Optional[torch.Tensor] = None, none_value=-2.0,
                       guidance_scale=None, y: Optional[torch.Tensor] = None, null_label: Optional[int] = None, timesteps=None, train_steps=None):
        """In-place DPM-Solver++ multistep sampling (mi355_ddpm_multistep_sample; with guidance_scale: mi355_ddpm_multistep_cfg_sample): one
        evaluation and one step launch per step, deterministic.  tables: as in ddpm_sample; coefs: (cx, c0, c1) of DDPM.dpm_solver_coefs(order)
        for the same chain.  cond: None (prior; an amortized net sees none_value) or the condition of an amortized net.  timesteps / train_steps
        (both or neither): where the steps sit in training time (a RespacedDDPM's timesteps and base_Ns); None: steps 0..Ns-1 of Ns.
        guidance_scale, y, null_label: as in ddpm_sample.  A guided batch beyond cfg_batch() runs in slices."""
        B = x.shape[0]
        if cond is not None and cond.shape != x.shape:
            raise ValueError("condition must have the shape of x")
        if guidance_scale is None and y is not None:
            raise NotImplementedError("ddpm_multistep takes class labels on the guided path only (guidance_scale=)")
        if (timesteps is None) != (train_steps is None):
            raise ValueError("timesteps and train_steps go together")
        tb, keep = self._ddpm_tables(tables)
        K = int(tb.Ns)
        steps = list(range(K)) if timesteps is None else [int(t) for t in timesteps]
        if len(steps) != K:
            raise ValueError("timesteps must have one entry per row of the (respaced) tables")
        try:
            cs = [torch.as_tensor(c, dtype=torch.float32).detach().to("cpu").contiguous() for c in coefs]
        except TypeError:
            raise ValueError("coefs must be the (cx, c0, c1) of DDPM.dpm_solver_coefs") from None
        if len(cs) != 3 or any(c.numel() != K for c in cs):
            raise ValueError("coefs must be (cx, c0, c1), one entry per step each")
        ms, keep_ms = self._multistep_schedule(tb, cs, steps, train_steps)
        opt = self._ddpm_options(_lib.DDIM, cond, 0, float(none_value))
        name, guide, mb = "mi355_ddpm_multistep_sample", None, B   # (the unguided call does not slice)
        if guidance_scale is not None:
            lab, _ = self._labels(y, B)
            w, wt, nl = self._guidance_args(guidance_scale, B, lab, cond, null_label)
            name, guide, mb = "mi355_ddpm_multistep_cfg_sample", (lab, nl, w, wt), self.cfg_batch()
        self._ddpm_loop(name, "mi355_ddpm_multistep_workspace_bytes", (int(guide is not None),), mb, x, cond, None, tb, opt, guide=guide, mid=(ms,))
        del keep, keep_ms
        return x

    def ddpm_shaped(self, x: torch.Tensor, tables: Dict[str, torch.Tensor], shaping, *, mode: int, cond: Optional[torch.Tensor] = None,
                    noise: Optional[torch.Tensor] = None, n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0, start_fraction=1.0, noise_condition=True,
                    pad_value=-2.0, none_value=-2.0, seed=0, guidance_scale=None, y: Optional[torch.Tensor] = None, null_label: Optional[int] = None,
                    timesteps=None, train_steps=None, ddim_sigma=None, walk=None, coefs=None):
        """In-place DDPM sampling with per-image shaping of every predictor step's data prediction (mi355_ddpm_shaped_sample): dynamic
        thresholding and guidance rescale.  shaping: DDPM.x0_shaping, a (quantile, max_threshold, rescale_phi) triple, or None (the unshaped
        loop, bit for bit).  coefs None: the arguments and the loops of ddpm_sample; coefs = (cx, c0, c1): those of ddpm_multistep (mode must
        be DDIM; no noise).  guidance_scale not None: the guided loops; a batch beyond cfg_batch() runs in slices (Philox: seed + slice)."""
        loop = {k: v for k, v in locals().items() if k not in ("self", "shaping")}   # x, tables and the keywords the three entry points share
        return self._ddpm_one_entry("ddpm_shaped", "mi355_ddpm_shaped_sample", "mi355_ddpm_shaped_workspace_bytes", (_lib.x0_shaping(shaping),), [], **loop)

    def ddpm_learned(self, x: torch.Tensor, tables: Dict[str, torch.Tensor], max_log=None, *, mode: int, times=None, cond: Optional[torch.Tensor] = None,
                     noise: Optional[torch.Tensor] = None, n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0, start_fraction=1.0, noise_condition=True,
                     pad_value=-2.0, none_value=-2.0, seed=0, guidance_scale=None, y: Optional[torch.Tensor] = None, null_label: Optional[int] = None,
                     timesteps=None, train_steps=None, ddim_sigma=None, walk=None, coefs=None):
        """In-place DDPM sampling of a learned-variance net (mi355_ddpm_lv_sample): the engine's net writes twice x's channels, eps then v, and
        the ancestral step's variance is the learned range between tables["posterior_log_variance_clipped"] and max_log ([K] floats: log(betas) of
        the chain, DDPM.max_log()).  max_log None: the fixed-variance loops on a net of x's channel count, bit for bit.  times ([K] floats, or
        None: the loops' own rule): the time the net sees at step k (DDPM.time of a from_betas chain).  Everything else: the arguments and the
        loops of ddpm_shaped (coefs: the multistep solver)."""
        loop = {k: v for k, v in locals().items() if k not in ("self", "max_log", "times")}
        var, keep = self._ddpm_variance(tables, max_log, times)
        return self._ddpm_one_entry("ddpm_learned", "mi355_ddpm_lv_sample", "mi355_ddpm_lv_workspace_bytes", (var,), keep, **loop)

    def ddpm_pred(self, x: torch.Tensor, tables: Dict[str, torch.Tensor], prediction, *, mode: int, shaping=None, max_log=None, times=None,
                  cond: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0,
                  start_fraction=1.0, noise_condition=True, pad_value=-2.0, none_value=-2.0, seed=0, guidance_scale=None,
                  y: Optional[torch.Tensor] = None, null_label: Optional[int] = None, timesteps=None, train_steps=None, ddim_sigma=None, walk=None,
                  coefs=None):
        """In-place DDPM sampling of a net whose output is "eps", "x0" or "v" (mi355_ddpm_pred_sample): every step forms the data prediction of
        the kind from the net's raw output and goes on as ddpm_sample / ddpm_multistep (coefs), ddpm_shaped (shaping) and ddpm_learned (max_log,
        times) do; "eps" gives their bits.  shaping together with max_log is refused by the library."""
        loop = {k: v for k, v in locals().items() if k not in ("self", "prediction", "shaping", "max_log", "times")}
        var, keep = self._ddpm_variance(tables, max_log, times)
        extra = (var, _lib.x0_shaping(shaping), _lib.DDPMPredictionC(_lib.prediction_kind(prediction)))
        return self._ddpm_one_entry("ddpm_pred", "mi355_ddpm_pred_sample", "mi355_ddpm_pred_workspace_bytes", extra, keep, **loop)

    def ddpm_nullspace(self, x: torch.Tensor, tables: Dict[str, torch.Tensor], y: torch.Tensor, op, lam, sigma=None, *, mode: int, prediction=None,
                       labels: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, seed=0, timesteps=None, train_steps=None,
                       ddim_sigma=None, walk=None):
        """In-place null-space (DDNM) restoration with the engine's unconditional net (mi355_ddpm_nullspace_sample): every step rectifies its data
        prediction against the measurement y of the operator op (mi355.ops.Ops.nullspace_op) with lam[k], then moves the state from it.  mode
        DDPM_PRIOR: the ancestral form with the noise std sigma[k] (DDPM.nullspace_coefs); DDIM: the DDIM(eta) form with ddim_sigma (None:
        deterministic), sigma must be None.  labels: class labels [B] of a class-conditional net.  prediction, noise, seed, timesteps / train_steps,
        ddim_sigma, walk: as in ddpm_pred (walk: DDNM's time travel, conditioning.repaint_walk).  A net that writes 2C channels is read in the DDIM
        form alone.  -> x"""
        B = x.shape[0]
        if not isinstance(op, _lib.NullspaceOpC):
            raise TypeError("op must be a NullspaceOpC (mi355.ops.Ops.nullspace_op)")
        if y is None:
            raise ValueError("y (the measurement) is needed")
        if y.shape[0] != B:
            raise ValueError("the measurement y must have x's batch size")
        if noise is not None and noise.shape[1:] != x.shape:
            raise ValueError("injected noise must be [n_draws, B, C, H, W]")
        tb, keep = self._ddpm_tables(tables)
        K = int(tb.Ns)
        ns = _lib.NullspaceScheduleC()
        ns.lam, t = _host_floats(lam, K, "lam", per="step")
        keep.append(t)
        if sigma is not None:
            ns.sigma, t = _host_floats(sigma, K, "sigma", per="step")
            keep.append(t)
        sched = self._ddpm_schedule(tables, timesteps, train_steps, ddim_sigma, walk)
        lab, _ = self._labels(labels, B)
        opt = self._ddpm_options(mode, y, 0)
        self._ddpm_loop("mi355_ddpm_nullspace_sample", "mi355_ddpm_nullspace_workspace_bytes", (), B, x, y, noise, tb, opt, seed=int(seed),
                        guide=(lab, 0, 0.0, None), head=lambda ls: (C.byref(op), _lab_ptr(ls)),
                        mid=(None if sched is None else sched[0], ns, _lib.DDPMPredictionC(_lib.prediction_kind(prediction))), draws=True)
        del keep
        return x

    @staticmethod
    def _ddpm_variance(tables, max_log, times):
        """-> (mi355_ddpm_variance, or None when neither max_log nor times is given; the host tensors it points into)."""
        K = int(tables["alphas_cumprod_prev"].numel())
        var, keep = _lib.DDPMVarianceC(int(max_log is not None), None, None), []
        for name, v in (("max_log", max_log), ("times", times)):
            if v is not None:
                ptr, t = _host_floats(v, K, name)
                keep.append(t)
                setattr(var, name, ptr)
        return (var if keep else None), keep

    def _ddpm_one_entry(self, who, entry, ws_fn, extra, keep_extra, *, x, tables, mode, cond, noise, n_corrector, delta, tmin, tmax, start_fraction,
                        noise_condition, pad_value, none_value, seed, guidance_scale, y, null_label, timesteps, train_steps, ddim_sigma, walk, coefs):
        """The entry points that sit over the six DDPM loops (mi355_ddpm_shaped_sample, mi355_ddpm_lv_sample, mi355_ddpm_pred_sample): one argument
        list, with the entry point's own structs `extra` (a tuple, in order; None: a null pointer) between the schedules and the noise.  The
        keywords are the public methods' own."""
        B = x.shape[0]
        if cond is not None and cond.shape != x.shape:
            raise ValueError("condition must have the shape of x")
        if guidance_scale is None and y is not None:
            raise NotImplementedError(f"{who} takes class labels on the guided path only (guidance_scale=)")
        tb, keep = self._ddpm_tables(tables)
        keep += keep_extra
        K = int(tb.Ns)
        sched = ms = None
        if coefs is not None:
            if ddim_sigma is not None or walk is not None or noise is not None:
                raise ValueError("the multistep solver (coefs=) is deterministic: it takes no ddim_sigma, walk or noise")
            if (timesteps is None) != (train_steps is None):
                raise ValueError("timesteps and train_steps go together")
            steps = list(range(K)) if timesteps is None else [int(t) for t in timesteps]
            cs = [torch.as_tensor(c, dtype=torch.float32).detach().to("cpu").contiguous() for c in coefs]
            if len(steps) != K or len(cs) != 3 or any(c.numel() != K for c in cs):
                raise ValueError("timesteps and coefs = (cx, c0, c1) must have one entry per row of the tables")
            ms, keep_ms = self._multistep_schedule(tb, cs, steps, train_steps)
            keep += keep_ms
        else:
            sched = self._ddpm_schedule(tables, timesteps, train_steps, ddim_sigma, walk)
        if noise is not None and noise.shape[1:] != x.shape:
            raise ValueError("injected noise must be [n_draws, B, C, H, W]")
        guided = guidance_scale is not None
        guide, mb = (None, 0, 0.0, None), B
        if guided:
            lab, _ = self._labels(y, B)
            w, wt, nl = self._guidance_args(guidance_scale, B, lab, cond, null_label)
            guide, mb = (lab, nl, w, wt), self.cfg_batch()
        opt = self._ddpm_options(mode, cond, 0, none_value, n_corrector, delta, tmin, tmax, start_fraction, noise_condition, pad_value)
        self._ddpm_loop(entry, ws_fn, (int(guided), int(ms is not None)), mb, x, cond, noise, tb, opt, seed=int(seed), guide=guide, flag=guided,
                        mid=(None if sched is None else sched[0], ms) + extra, draws=True)
        del keep
        return x

    def ddpm_vlb(self, x0: torch.Tensor, tables: Dict[str, torch.Tensor], logs: Dict[str, torch.Tensor], *, learned: bool, times=None,
                 cond: Optional[torch.Tensor] = None, y: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None, seed=None, cdf="exact",
                 clip_denoised=True, none_value=-2.0, prediction=None):
        """The variational bound of the engine's net on data x0 [B, C, H, W] in [-1, 1] (mi355_ddpm_vlb): all K steps of the chain `tables`
        describes in ONE library call per batch.  logs: the [K] log-variance tables of DDPM.vlb_log_variances - "true_log", and "model_log"
        (fixed variance) or "min_log" and "max_log" (learned: the net writes twice x0's channels).  times ([K] floats, or None: k / K): the time
        the net sees at step k.  cond: the condition of a 2C-input net (None: such a net sees none_value).  noise: [K, B, C, H, W] injected draws
        (draw j belongs to step K-1-j), or None: device Philox at `seed`.  cdf: "exact" or "tanh".
        -> (terms [B, K, 3] = vb, xstart_mse, mse per step; summary [B, 2] = prior_bpd, total_bpd).  A batch beyond max_batch() runs in slices
        (Philox: seed + slice).  prediction (None or "eps": mi355_ddpm_vlb; "x0", "v": mi355_ddpm_vlb_pred): what the net's output stands for -
        x0_hat comes from it, and the third term is the squared error against the kind's training target."""
        pred = _lib.DDPMPredictionC(_lib.prediction_kind(prediction))
        if x0.dim() != 4:
            raise ValueError("x0 must be [B, C, H, W]")
        if cond is not None and cond.shape != x0.shape:
            raise ValueError("condition must have the shape of x0")
        if cdf not in ("exact", "tanh"):
            raise ValueError(f'cdf must be "exact" or "tanh", got {cdf!r}')
        B = x0.shape[0]
        tb, keep = self._ddpm_tables(tables)
        K = int(tb.Ns)
        opt = _lib.VLBOptionsC(int(bool(learned)), int(cdf == "tanh"), int(bool(clip_denoised)), None, None, None, None, None, float(none_value), 0)
        need = ("true_log", "min_log", "max_log") if learned else ("true_log", "model_log")
        for name, v in [(n, logs.get(n)) for n in need] + [("times", times)]:
            if v is None:
                if name == "times":
                    continue
                raise ValueError(f"logs[{name!r}] is needed ({'learned' if learned else 'fixed'} variance): DDPM.vlb_log_variances builds it")
            ptr, t = _host_floats(v, K, name)
            keep.append(t)
            setattr(opt, name, ptr)
        if noise is not None and (noise.dim() != 5 or tuple(noise.shape[1:]) != tuple(x0.shape)):
            raise ValueError(f"noise must be [draws, *x0.shape], got {tuple(noise.shape)}")
        lab, _ = self._labels(y, B)
        terms = torch.empty(B, K, 3, device=self.device, dtype=torch.float32)
        summary = torch.empty(B, 2, device=self.device, dtype=torch.float32)
        self._fwd_state = None
        seed = 0 if seed is None else int(seed)
        name = "mi355_ddpm_vlb" if pred.kind == 0 else "mi355_ddpm_vlb_pred"
        for n, (xs, cn, ls, tm, sm), (nz,), _, sd in self._sliced(B, self.max_batch(), rows=(x0, cond, lab, terms, summary), cols=(noise,), seed=seed):
            opt.seed = sd
            ws, wsb = self._workspace_sized("mi355_ddpm_vlb_workspace_bytes", n)
            check(getattr(self.L, name)(self.handle, self._chk(xs, "x0"), xs.shape[1], self._ptr(cn, "condition"), _lab_ptr(ls), C.byref(tb), C.byref(opt),
                                        *(() if pred.kind == 0 else (C.byref(pred),)), *self._noise_args(nz), self._chk(tm, "terms"),
                                        self._chk(sm, "summary"), n, ws, wsb, self._stream()), name)
        del keep
        return terms, summary

    def _ddpm_cfg_call(self, x, tables, mode, cond, lab, null_label, w, wt, noise, o, sched=None):
        """One mi355_ddpm_cfg_sample (sched: mi355_ddpm_cfg_sample_sched) call (a batch within cfg_batch())."""
        B = x.shape[0]
        tb, keep = self._ddpm_tables(tables)
        opt = self._ddpm_options(mode, cond, o["seed"], o["none_value"], o["n_corrector"], o["delta"], o["tmin"], o["tmax"])
        self._fwd_state = None
        ws, wsb = self._workspace_sized("mi355_ddpm_cfg_workspace_bytes", B)
        name = "mi355_ddpm_cfg_sample" if sched is None else "mi355_ddpm_cfg_sample_sched"
        self._ddpm_call(name, x, cond, tb, opt, B, ws, wsb, guide=(lab, null_label, w, wt), mid=() if sched is None else (sched[0],),
                        noise=self._noise_args(noise))
        del keep

    @staticmethod
    def _ddpm_options(mode, cond, seed, none_value=-2.0, n_corrector=0, delta=0.1, tmin=1e-5, tmax=1.0, start_fraction=1.0, noise_condition=True,
                      pad_value=-2.0):
        """mi355_ddpm_options.  The defaults are what the guided ddpm_sample path and the multistep solver pass for the fields they do not take."""
        return _lib.DDPMOptionsC(mode, n_corrector, delta, tmin, tmax, start_fraction, int(noise_condition), pad_value, none_value, int(cond is None), seed)

    def _ddpm_loop(self, name, ws_fn, ws_tail, mb, x, cond, noise, tb, opt, seed=None, guide=None, flag=None, mid=(), draws=False, head=None):
        """The calls of the DDPM entry point `name` on a batch run at most mb images at a time, each on a workspace of ws_fn(batch, *ws_tail).  seed:
        the Philox seed of the batch, the slices draw from seed + slice index (None: opt's own).  draws: the entry point takes injected noise.
        guide, flag, mid, head: see _ddpm_call."""
        lab, nl, w, wt = guide or (None, 0, 0.0, None)
        self._fwd_state = None
        for n, (xs, cn, ls, wl), (nz,), _, sd in self._sliced(x.shape[0], mb, rows=(x, cond, lab, wt), cols=(noise,), seed=seed):
            if sd is not None:
                opt.seed = sd
            ws, wsb = self._workspace_sized(ws_fn, n, *ws_tail)
            self._ddpm_call(name, xs, cn, tb, opt, n, ws, wsb, guide=guide and (ls, nl, w, wl), flag=flag, mid=mid,
                            noise=self._noise_args(nz) if draws else (), head=head)

    def _ddpm_call(self, name, x, cond, tb, opt, B, ws, wsb, guide=None, flag=None, mid=(), noise=(), last=(), head=None):
        """One call of the DDPM entry point `name`, in the argument order they share: handle, x, C, cond, [labels, null_label, (guided flag,) w,
        per-image scales,] tables, options, mid, [noise, n_draws,] batch, workspace, stream, last.  guide: (labels, null_label, w, scales) where the
        entry point takes guidance, flag: its guided flag where it has one.  mid: the schedules and the entry point's own structs, each a struct
        or None (a null pointer); noise: _noise_args where the entry point draws; last: the feature cache or the tile plan.  head (with guide =
        (labels, ...)): what the entry point takes between the condition and the tables in place of the guidance arguments, a function of the
        (sliced) labels -> tuple (mi355_ddpm_nullspace_sample: the operator and the labels; its measurement rides in the condition's place)."""
        g = ()
        if head is not None:
            g = head(guide[0] if guide is not None else None)
        elif guide is not None:
            lab, nl, w, wt = guide
            g = (_lab_ptr(lab), int(nl), *(() if flag is None else (int(flag),)), float(w), self._ptr(wt, "guidance_scale"))
        check(getattr(self.L, name)(self.handle, self._chk(x, "x"), x.shape[1], self._ptr(cond, "condition"), *g, C.byref(tb), C.byref(opt),
                                    *(None if s is None else C.byref(s) for s in mid), *noise, B, ws, wsb, self._stream(),
                                    *(C.byref(s) for s in last)), name)

    def _noise_args(self, noise):
        return (self._ptr(noise, "noise"), noise.shape[0] if noise is not None else 0)

    @staticmethod
    def _multistep_schedule(tb, coefs, timesteps, train_steps):
        """coefs: the (cx, c0, c1) CPU fp32 tensors, timesteps: the K training indices  =>  (mi355_multistep_schedule, what it points into)."""
        K = int(tb.Ns)
        ms = _lib.MultistepScheduleC()
        steps_arr = (C.c_int32 * max(1, K))(*timesteps)
        ms.steps, ms.train_steps = C.cast(steps_arr, C.POINTER(C.c_int32)), K if train_steps is None else int(train_steps)
        ms.cx, ms.c0, ms.c1 = (C.cast(c.data_ptr(), C.POINTER(C.c_float)) for c in coefs)
        return ms, list(coefs) + [steps_arr]

    @staticmethod
    def _ddpm_tables(tables):
        """name -> CPU fp32 tensor [Ns]  =>  (mi355_ddpm_tables, the tensors it points into)."""
        tb = _lib.DDPMTablesC()
        keep = []
        Ns = None
        fp = C.POINTER(C.c_float)
        for name, _ in _lib.DDPMTablesC._fields_[1:]:
            v = tables[name].detach().to("cpu", torch.float32).contiguous()
            Ns = v.numel() if Ns is None else Ns
            if v.numel() != Ns:
                raise ValueError("DDPM tables must all have length Ns")
            keep.append(v)
            setattr(tb, name, C.cast(v.data_ptr(), fp))
        tb.Ns = Ns
        return tb, keep

    @staticmethod
    def _ddpm_schedule(tables, timesteps, train_steps, ddim_sigma, walk):
        """-> None (no schedule given), or (mi355_ddpm_schedule, the host arrays it points into)."""
        if timesteps is None and train_steps is None:
            if ddim_sigma is not None or walk is not None:
                raise ValueError("ddim_sigma and walk belong to a scheduled call: give timesteps and train_steps (DDPM.respace)")
            return None
        if timesteps is None or train_steps is None:
            raise ValueError("timesteps and train_steps go together")
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        sd = _lib.DDPMScheduleC()
        K = len(timesteps)
        if K != tables["alphas_cumprod_prev"].numel():
            raise ValueError("timesteps must have one entry per row of the (respaced) tables")
        keep = [(C.c_int32 * max(1, K))(*[int(t) for t in timesteps])]
        sd.steps, sd.train_steps = C.cast(keep[0], ip), int(train_steps)
        if ddim_sigma is not None:
            sd.ddim_sigma, sg = _host_floats(ddim_sigma, K, "ddim_sigma", per="step")
            keep.append(sg)
        if walk is not None:
            wl = (C.c_int32 * max(1, len(walk)))(*[int(v) for v in walk])
            keep.append(wl)
            sd.walk, sd.n_walk = C.cast(wl, ip), len(walk)
            if any(b > a for a, b in zip(walk, list(walk)[1:])):   # upward moves: q(x_k | x_{k-1}) = sqrt(alphas_k) x + sqrt(betas_k) z
                ra = torch.sqrt(tables["alphas"].detach().to("cpu", torch.float32)).contiguous()
                rb = torch.sqrt(tables["betas"].detach().to("cpu", torch.float32)).contiguous()
                keep += [ra, rb]
                sd.renoise_a, sd.renoise_b = C.cast(ra.data_ptr(), fp), C.cast(rb.data_ptr(), fp)
        return sd, keep
