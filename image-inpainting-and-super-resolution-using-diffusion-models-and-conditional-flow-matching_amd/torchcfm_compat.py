"""Stand-ins for the two un-vendored third-party front-ends the reference's cifar10/ and mnist/ scripts
import, so those scripts' sampler call sites work unchanged on the MI355X backend:

  torchcfm.models.unet.unet.UNetModelWrapper   (cifar10/train_cifar10.py:22,92-101; compute_fid.py:16,39-48)
  torchdyn.core.NeuralODE                      (cifar10/utils_cifar.py:4,34-39; compute_fid.py:14,69-70)

Neither package is in /root/reference (versions unpinned; weight URLs point at torchcfm 1.0.4); their
published behaviour is restated from the reference's call sites: constructor keywords, the
`model(t, x, y=None)` call convention with scalar or [B] `t`, and `trajectory(x, t_span)` returning all
len(t_span) states of a fixed-step Euler integration.  `InPaintModelWrapper` / `SuperResModelWrapper` are
the author's unpublished torchcfm edits (mnist/train_mnist.py:34, train_mnist_hy.py:36); their semantics
(channel-concat of the condition / of the bilinearly upsampled low-res image) are inferred from the
keyword arguments at mnist/utils_mnist.py:97 and mnist/utils_mnist_hy.py:82 - "parity unpinned".
"""
from __future__ import annotations

from typing import Optional

import torch

from image_diffusion.unet import UNetModel
from mi355.ode import AB_SOLVERS, RK_SOLVERS
from mi355.ops import default_ops


def _default_mult(image_size):
    table = {512: (0.5, 1, 1, 2, 2, 4, 4), 256: (1, 1, 2, 2, 4, 4), 128: (1, 1, 2, 3, 4), 64: (1, 2, 3, 4), 32: (1, 2, 2, 2),
             28: (1, 2, 2)}
    if image_size not in table:
        raise ValueError(f"unsupported image size: {image_size}")
    return table[image_size]


class UNetModelWrapper(UNetModel):
    """torchcfm UNetModelWrapper: dim=(C,H,W), attention_resolutions as a string of resolutions.  The stand-in of the cifar10/ and mnist/
    call sites, which build no label embedding: class_cond=True with num_classes set is refused here (ClassCondUNetModelWrapper builds it)."""

    _class_cond_ok = False   # ClassCondUNetModelWrapper: label_emb is built

    def __init__(self, dim, num_channels, num_res_blocks, channel_mult=None, learn_sigma=False, class_cond=False, num_classes=None,
                 use_checkpoint=False, attention_resolutions="16", num_heads=1, num_head_channels=-1, num_heads_upsample=-1,
                 use_scale_shift_norm=False, dropout=0, resblock_updown=False, use_fp16=False, use_new_attention_order=False,
                 in_channels: Optional[int] = None, precision: Optional[str] = None):
        image_size = dim[-1]
        channel_mult = _default_mult(image_size) if channel_mult is None else tuple(channel_mult)
        attention_ds = tuple(image_size // int(res) for res in str(attention_resolutions).split(","))
        # torchcfm: `num_classes if class_cond else None` - a label embedding exists only when class_cond is set AND a class count is
        # given (conditional_mnist.ipynb: class_cond=True, num_classes=10).  The mnist/ call sites pass class_cond=True WITH
        # num_classes=None (mnist/train_mnist.py:262-267, train_mnist2.py:350-355, train_mnist_hy.py:312-318, train_mnist_hy2.py:313-318),
        # i.e. an unconditional network.
        num_classes = num_classes if class_cond else None
        if num_classes is not None and not self._class_cond_ok:
            raise NotImplementedError("UNetModelWrapper stands in for the cifar10/ and mnist/ call sites and builds no label_emb; the "
                                      "class-conditional torchcfm model (class_cond=True, num_classes=K, as conditional_mnist.ipynb builds it) "
                                      "is torchcfm_compat.ClassCondUNetModelWrapper")
        super().__init__(image_size=image_size, in_channels=dim[0] if in_channels is None else in_channels,
                         model_channels=num_channels, out_channels=(dim[0] if not learn_sigma else dim[0] * 2),
                         num_res_blocks=num_res_blocks, attention_resolutions=attention_ds, dropout=dropout,
                         channel_mult=channel_mult, num_classes=num_classes, use_checkpoint=use_checkpoint, use_fp16=use_fp16,
                         num_heads=num_heads, num_head_channels=num_head_channels, num_heads_upsample=num_heads_upsample,
                         use_scale_shift_norm=use_scale_shift_norm, resblock_updown=resblock_updown,
                         use_new_attention_order=use_new_attention_order, precision=precision)

    def _t(self, t, x):
        if isinstance(t, (int, float)) or (isinstance(t, torch.Tensor) and t.dim() == 0 and not t.is_cuda):
            return float(t)          # one host-side time for the batch: the engine broadcasts it (no device tensor, no ATen kernel)
        t = torch.as_tensor(t, device=x.device).float()
        while t.dim() > 1:
            t = t[:, 0]
        if t.dim() == 0:
            t = t.repeat(x.shape[0])
        return t

    @staticmethod
    def _c(t):
        return t if isinstance(t, float) else t.contiguous()

    @torch.no_grad()
    def forward(self, t, x, y=None, *args, guidance_scale=None, null_label=None, **kwargs):
        """torchcfm: model(t, x, y).  A class-conditional model (num_classes set) needs y, the labels [B]; without num_classes y is ignored
        (the mnist/ call sites' class_cond=True, num_classes=None networks).
        guidance_scale (a float or a [B] tensor; None: the plain forward): the classifier-free-guided field v_u + w (v_c - v_u), v_u at
        null_label (default: the last class), from one evaluation at twice the batch - odeint_dopri5(lambda t, x: model(t, x, y,
        guidance_scale=w, null_label=K), ...)."""
        if self.num_classes is None:
            y = None
        elif y is None:
            raise ValueError("y (class labels) is required: this model was built with class_cond=True and num_classes="
                             f"{self.num_classes} (torchcfm asserts (y is not None) == (num_classes is not None))")
        if not x.is_cuda:
            return super().forward(x, t)     # raises MI355BackendError (no CPU path)
        if guidance_scale is not None:
            return self.engine(x.device).forward(x.float().contiguous(), self._c(self._t(t, x)), y=y, guidance_scale=guidance_scale,
                                                 null_label=null_label)
        return self.engine(x.device).forward(x.float().contiguous(), self._c(self._t(t, x)), y=y)


class ClassCondUNetModelWrapper(UNetModelWrapper):
    """torchcfm's UNetModelWrapper built class-conditional, the model of conditional_mnist.ipynb (`from torchcfm.models.unet import
    UNetModel`; `UNetModel(dim=(1, 28, 28), num_channels=32, num_res_blocks=1, num_classes=10, class_cond=True)`): the same constructor,
    label_emb.weight [num_classes, 4 * num_channels] (N(0, 1) init), and model(t, x, y) with y, the labels [B], required.  Sample it with
    odeint_dopri5(lambda t, x: model(t, x, y), ...), model.engine().cfm_euler(x, t_span, y=y), or NeuralODE(GuidedVectorField(model, y=y,
    guidance_scale=w)): NeuralODE itself has no labels to pass, the GuidedVectorField carries them."""

    _class_cond_ok = True


class InPaintModelWrapper(UNetModelWrapper):
    """model.forward(x, t, con=con): the -2-sentinel condition image is concatenated on the channel axis."""

    def __init__(self, dim, *a, **kw):
        super().__init__(dim, *a, in_channels=2 * dim[0], **kw)

    @torch.no_grad()
    def forward(self, x, t, con=None, **kwargs):
        eng = self.engine(x.device)
        return eng.forward(x.float().contiguous(), self._c(self._t(t, x)), cond=con.float().contiguous())


class SuperResModelWrapper(UNetModelWrapper):
    """model.forward(x, t, low_res=low_res): low_res is bilinearly upsampled to x's size and concatenated
    (the guided-diffusion SuperResModel convention)."""

    def __init__(self, dim, *a, **kw):
        super().__init__(dim, *a, in_channels=2 * dim[0], **kw)

    def upsample(self, low_res, size):
        """bilinear, align_corners=False (mnist/utils_mnist_hy.py:18-28 is the matching downsample): the HIP resize kernel"""
        return default_ops.resize_bilinear(low_res.float().contiguous(), size)

    @torch.no_grad()
    def forward(self, x, t, low_res=None, **kwargs):
        up = self.upsample(low_res, (x.shape[2], x.shape[3]))
        eng = self.engine(x.device)
        return eng.forward(x.float().contiguous(), self._c(self._t(t, x)), cond=up)


class GuidedVectorField:
    """A vector field with what a NeuralODE call site cannot pass: class labels y [B] and / or a condition con [B, Cc, H, W], and a
    classifier-free guidance scale (a float or a [B] tensor).  f(t, x) = v_u + w (v_c - v_u), v_u at null_label (default: the last class)
    and / or the none_value-filled condition.  NeuralODE.trajectory recognises it: with a fixed-step solver the whole guided integration is
    one library call (UNetEngine.cfm_euler / cfm_rk, mi355_cfm_cfg_sample); dopri5 calls it per evaluation."""

    def __init__(self, model, y=None, con=None, guidance_scale=1.0, null_label=None, none_value=-2.0):
        if y is None and con is None:
            raise ValueError("GuidedVectorField needs class labels (y) and / or a condition (con)")
        self.model, self.y, self.con = model, y, con
        self.guidance_scale, self.null_label, self.none_value = guidance_scale, null_label, float(none_value)

    def _kw(self, device):
        con = self.con.to(device).float().contiguous() if self.con is not None else None
        return dict(cond=con, y=self.y.to(device) if self.y is not None else None, guidance_scale=self.guidance_scale,
                    null_label=self.null_label, none_value=self.none_value)

    @torch.no_grad()
    def __call__(self, t, x, *args, **kwargs):
        return self.model.engine(x.device).forward(x.float().contiguous(), self.model._c(self.model._t(t, x)), **self._kw(x.device))


class NeuralODE:
    """torchdyn.core.NeuralODE front-end: solver="euler" (fixed step), "midpoint", "heun2", "rk4", "rk4_38" (fixed-step explicit
    Runge-Kutta, the tableaus of mi355.ode.TABLEAUS: "rk4" the classical one, "rk4_38" the 3/8 rule), "ab2", "ab3", "ab4" (Adams-Bashforth,
    mi355.ode.AB_SOLVERS: one evaluation per step after a Runge-Kutta start; mi355_cfm_ab_sample / mi355.ode.AdamsBashforth) or "dopri5"
    (adaptive, mi355.ode.Dopri5).

    trajectory(x, t_span) -> Tensor[len(t_span), *x.shape], one step per interval of t_span for the fixed-step solvers.  With a
    UNetModelWrapper vector field these run the whole integration inside libmi355_sampler (mi355_cfm_euler_sample /
    mi355_cfm_rk_sample); any other callable f(t, x[, args]) is driven step by step from the host with the HIP update kernels
    (mi355.ode.FixedStepRK for the Runge-Kutta methods).  dopri5 is one continuous adaptive solve with dense output at the requested times.

    cache_interval / cache_branch (BUILD-DEFINED EXTENSION; None: untouched): feature reuse across the Euler steps of a UNetModelWrapper
    (DeepCache: one full U-Net evaluation in cache_interval steps, the cache_branch outermost block pairs recomputed at every step;
    UNetEngine.cfm_euler).  solver="euler" on the device only; any other solver or vector field refuses it.

    tiling (BUILD-DEFINED EXTENSION; None: untouched; an image_diffusion.sampling.Tiling): x is a canvas [B, C, Hc, Wc] larger than the model's
    frame, every Euler step evaluates the model on overlapping windows and blends them (MultiDiffusion; UNetEngine.cfm_euler(tiling=)).
    solver="euler" on a UNetModelWrapper on the device only; not with cache_interval / cache_branch."""

    RK_SOLVERS = RK_SOLVERS   # mi355.ode: every fixed-step tableau name but "euler"

    def __init__(self, vector_field, solver="euler", sensitivity="adjoint", atol=1e-4, rtol=1e-4, cache_interval=None, cache_branch=None, tiling=None,
                 **kwargs):
        if solver not in ("euler", "dopri5") + self.RK_SOLVERS + AB_SOLVERS:
            raise NotImplementedError(f"solver={solver!r}: only 'euler', 'dopri5', {self.RK_SOLVERS} and {AB_SOLVERS} are built")
        self.cache = {}
        if cache_interval is not None or cache_branch is not None:
            if solver != "euler" or type(vector_field) is not UNetModelWrapper:
                raise NotImplementedError("cache_interval / cache_branch (feature reuse) are built for solver='euler' on a UNetModelWrapper "
                                          "(not for the guided, Runge-Kutta, Adams-Bashforth or adaptive solvers, nor for other callables)")
            self.cache = dict(cache_interval=1 if cache_interval is None else cache_interval, cache_branch=cache_branch)
        if tiling is not None:
            if solver != "euler" or type(vector_field) is not UNetModelWrapper:
                raise NotImplementedError("tiling is built for solver='euler' on a UNetModelWrapper (not for the guided, Runge-Kutta, "
                                          "Adams-Bashforth or adaptive solvers, nor for other callables)")
            if self.cache:
                raise NotImplementedError("tiling together with cache_interval / cache_branch is not built")
            self.cache = dict(tiling=tiling)   # (the keyword the Euler call below takes in its place)
        self.vf = vector_field
        self.solver = solver
        self.atol, self.rtol = atol, rtol

    def to(self, *a, **k):
        return self

    def _call(self, t, x):
        # the library's own wrappers take the host scalar as it is; any other vector field gets the 0-dim tensor torchdyn passes
        tt = float(t) if isinstance(self.vf, (UNetModelWrapper, GuidedVectorField)) else torch.tensor(float(t), device=x.device, dtype=torch.float32)
        try:
            return self.vf(tt, x)
        except TypeError:
            return self.vf(tt, x, None)  # torchdyn passes `args` to 3-argument vector fields (mnist/utils_mnist2.py:120)

    @torch.no_grad()
    def trajectory(self, x, t_span):
        ts = [float(v) for v in torch.as_tensor(t_span).detach().cpu().tolist()]
        x = x.detach().clone().float().contiguous()
        if self.solver == "dopri5":
            # torchdyn's adaptive path (mnist/utils_mnist.py:63-68): states at every requested time; callers index [-1]
            from mi355.ode import Dopri5

            solver = Dopri5(lambda t, y: [self._call(t, y[0])], self.rtol, self.atol)
            states = solver.integrate_times([x], ts)   # one continuous adaptive solve, dense output at every requested time
            return torch.stack([x] + [s[0] for s in states])
        if isinstance(self.vf, GuidedVectorField) and x.is_cuda:   # fixed-step and guided: one library call
            eng = self.vf.model.engine(x.device)
            kw = self.vf._kw(x.device)
            if self.solver == "euler":
                return eng.cfm_euler(x, ts, keep_traj=True, **kw)[1]
            if self.solver in AB_SOLVERS:
                return eng.cfm_ab(x, ts, self.solver, keep_traj=True, **kw)[1]
            return eng.cfm_rk(x, ts, self.solver, keep_traj=True, **kw)[1]
        if self.solver in AB_SOLVERS:   # Adams-Bashforth: one library call on the device, the host class for any other callable
            if type(self.vf) is UNetModelWrapper and x.is_cuda:
                return self.vf.engine(x.device).cfm_ab(x, ts, self.solver, keep_traj=True)[1]
            from mi355.ode import AdamsBashforth

            states = AdamsBashforth(lambda t, y: [self._call(t, y[0])], self.solver).integrate_times([x], ts)
            return torch.stack([x] + [s[0] for s in states])
        if self.solver in self.RK_SOLVERS:
            if type(self.vf) is UNetModelWrapper and x.is_cuda:
                _, traj, _ = self.vf.engine(x.device).cfm_rk(x, ts, self.solver, keep_traj=True)
                return traj
            from mi355.ode import FixedStepRK

            states = FixedStepRK(lambda t, y: [self._call(t, y[0])], self.solver).integrate_times([x], ts)
            return torch.stack([x] + [s[0] for s in states])
        if type(self.vf) is UNetModelWrapper and x.is_cuda:
            _, traj, _ = self.vf.engine(x.device).cfm_euler(x, ts, keep_traj=True, **self.cache)
            return traj
        if self.cache:
            from mi355._lib import MI355BackendError
            raise MI355BackendError("feature reuse (cache_interval) and tiling run inside the device loop: x must be a device tensor")
        out = [x.clone()]
        for k in range(len(ts) - 1):
            t = ts[k] if isinstance(self.vf, UNetModelWrapper) else torch.tensor(ts[k], device=x.device, dtype=torch.float32)
            try:
                v = self.vf(t, x)
            except TypeError:
                v = self.vf(t, x, None)  # torchdyn passes `args` to 3-argument vector fields (mnist/utils_mnist2.py:120)
            default_ops.euler_step_(x, v.float().contiguous(), ts[k + 1] - ts[k])
            out.append(x.clone())
        return torch.stack(out)
