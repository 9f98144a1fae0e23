"""CPU: the fp64 references, input classes, case lists and error budgets of tests/test_gpu_embed_ops.py, proved without a GPU.

The embedding path (csrc/embed.hip) in the reference model's own words:
    timestep_embedding (nn.py:97-115)   cat(cos(t f), sin(t f)), f_k = exp(-ln(max_period) k / half), half = dim // 2, a zero column for odd dim;
    time_embed (unet.py:564-569)        Linear, SiLU, Linear               -> two calls of the linear kernels (out_act, then none);
    emb_layers (unet.py:297-305)        SiLU, Linear                       -> in_act; batched over every ResBlock of a forward;
    label_emb (unet.py:572)             emb = time_embed(.) + label_emb(y) -> emb_gather, or fused: silu(h + label_emb[y]) W^T + b.
Every reference here is plain fp64 torch on the fp32 values the kernel reads.

Budgets (none is a number chosen in advance; nothing is fitted to a kernel):
  linear ops   e = |got - ref64| / (sum_k |act(x_k) w_kj| + |bias_j|), the denominator in fp64; budget(K) = 4 x the largest e of the fp32 eager
               restatement (F.silu / F.linear in fp32 on the CPU) over every run of the GPU test with that K: three input classes, four
               activation settings, bias present and absent.  The factor 4 is the GroupNorm tests' margin (tests/test_gn_ref_cpu.py): another
               summation order, the device's expf.
  timestep     budget(class) = 4 x the worst absolute error of the fp32 eager restatement of nn.py:107-115 against fp64 over every element of
               that class of |t| in every case of the GPU test: flow times in [0, 1], |t| <= 8, DDPM steps up to 999, beyond the table up to 1e4.
  pack         bit-identical to torch's round-to-nearest-even cast; unpack and gather: exact copies.
  pool         |got - ref64| <= u_T |ref64| + 3 u32 mean |in|: one store rounding (u_T = 0, 2^-8, 2^-11 for fp32, bf16, fp16) and the three fp32
               additions (u32 = 2^-24); the reference is AvgPool2d(2) in fp64 of the values the kernel reads.

Measured (the fp32 eager restatement against fp64; the budget is 4 x these, computed afresh wherever the tests run):
  linear, largest normalised error per K over both linear ops:
    K      4        32       36       48       96       100      128      512      1024     1028     2048     4096
    e_ref  2.8e-07  3.2e-07  4.4e-07  4.3e-07  4.2e-07  5.2e-07  4.7e-07  1.1e-07  2.2e-07  2.5e-07  1.6e-07  1.0e-07
    (the large K depend on the host's GEMM blocking: the host of the MI355X gave 2.8e-07, 1.6e-07, 2.0e-07, 2.1e-07, 1.2e-07 from K = 512 on)
  timestep embedding, worst absolute error per class of |t|:
    flow 7.6e-08   |t| <= 8 5.3e-07   DDPM steps 6.6e-05   beyond the table 6.5e-04
(the same numbers are in DESIGN.md, "Embedding path: measured error").

This module shows that (i) the references are the oracle's functions, (ii) the fp32 restatement in the KERNELS' summation order (slab kernels:
fmaf chains over blocks of 32 k, added up in order; small kernel: four K quarters merged at the end) passes every budget, so the budgets can
be met - a single chain over K = 2048, the slab kernels' order before this test, does not (1.12 x the budget) - and (iii) each of twelve mutants - the
ways these kernels can be wrong - breaks its budget on the cases listed with it, so no budget is wide enough to hide one.
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mi355.synth import rand_uniform, randn
from oracle import unet_ref

U32 = 2.0 ** -24
U_STORE = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}   # as U16 of tests/test_gpu_gn_ops.py
INT32_MIN = -2 ** 31


def silu64(v):
    return v * torch.sigmoid(v)


# ---- timestep embedding -----------------------------------------------------------------------------------------------------------------
def timestep_embedding64(t, dim, max_period=10000.0):
    """nn.py:107-115 in fp64 on the fp32 times."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64) / max(half, 1))
    args = t.double()[:, None] * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


def timestep_embedding32_eager(t, dim, max_period=10000.0):
    """nn.py:107-115 as written: fp32."""
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(start=0, end=half, dtype=torch.float32) / half)
    args = t[:, None].float() * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


T_CLASSES = ("flow", "small", "ddpm", "beyond")
T_LIMITS = (1.0, 8.0, 999.0, 1e4)
T_FIXED = {"flow": [0.0, 1.0, 0.5, -0.25, 0.00390625, 0.999], "small": [8.0, -3.0, 2.5, 7.75, 1.0000001],
           "ddpm": [999.0, 9.0, -250.0, 500.5, 998.0, 37.0], "beyond": [1e4, 1000.0, -5000.0, 2500.25, 9999.0]}
T_DIMS = (2, 32, 33, 128, 192, 255)
T_BATCHES = (1, 5, 300)
T_PERIODS = (10000.0, 100.0)


def t_class(t):
    """Class index of every time by |t|."""
    a = t.abs().double()
    return sum((a > lim).long() for lim in T_LIMITS[:-1])


def make_times(B, ci):
    """B fp32 times: the fixed values of the four classes in turn (0, a negative and a fractional time, 999 and 1e4 among them), rotated by the
    case index so that B = 1 and B = 5 see every class over the cases, then for larger B uniform draws from each class's range."""
    fixed = [T_FIXED[c][(i + ci) % len(T_FIXED[c])] for i in range(6) for c in T_CLASSES]
    fixed = fixed[ci % 4:] + fixed[:ci % 4]
    if B <= len(fixed):
        return torch.tensor(fixed[:B], dtype=torch.float32)
    n = B - len(fixed)
    lo = (0.0,) + T_LIMITS[:-1]
    draws = torch.cat([rand_uniform(900 + ci * 4 + k, lo[k], T_LIMITS[k], (n + 3) // 4) * (1.0 if k % 2 else -1.0) ** (ci % 2) for k in range(4)])
    return torch.cat([torch.tensor(fixed, dtype=torch.float32), draws[:n]]).contiguous()


def timestep_cases():
    """(case index, t, dim, max_period) of the GPU test: every dim x batch x max_period."""
    out = []
    for dim in T_DIMS:
        for B in T_BATCHES:
            for mp in T_PERIODS:
                out.append((len(out), make_times(B, len(out)), dim, mp))
    return out


def class_errors(got, want, t):
    """Worst |got - want| per class of |t| -> list of four (0.0 where the class is absent)."""
    err = (got.double() - want).abs().amax(dim=1)
    cls = t_class(t)
    return [float(err[cls == k].max()) if bool((cls == k).any()) else 0.0 for k in range(4)]


@functools.lru_cache(maxsize=None)
def timestep_eager_errors():
    worst = [0.0] * 4
    for _, t, dim, mp in timestep_cases():
        e = class_errors(timestep_embedding32_eager(t, dim, mp), timestep_embedding64(t, dim, mp), t)
        worst = [max(a, b) for a, b in zip(worst, e)]
    return tuple(worst)


def timestep_budgets():
    return tuple(4.0 * e for e in timestep_eager_errors())


def check_timestep(got, t, dim, mp, tag, report=None):
    """-> worst error / budget over the classes present."""
    want = timestep_embedding64(t, dim, mp)
    errs, buds = class_errors(got, want, t), timestep_budgets()
    if report is not None:
        report(f"   EMBSTAT {tag}: " + " ".join(f"{c} {e:.2e}/{b:.2e}" for c, e, b in zip(T_CLASSES, errs, buds)))
    for c, e, b in zip(T_CLASSES, errs, buds):
        assert e <= b, f"{tag}: class {c}: |err| {e:.3e} > budget {b:.3e}"
    if dim % 2:
        assert bool((got[:, -1] == 0).all()), f"{tag}: the pad column of an odd dim is not exactly 0"
    return max(e / b for e, b in zip(errs, buds))


# ---- the linears --------------------------------------------------------------------------------------------------------------------------
LINEAR_CLASSES = ("count", "normal", "wide")


def class_tensor(cls, seed, *shape):
    """count: |v| in [0.5, 1.5] with random signs (every term counts); normal: N(0, 1); wide: N(0, 1) with every seventh entry scaled out to
    +-100 (SiLU meets both ends of expf: exp(100) overflows fp32)."""
    if cls == "count":
        return (rand_uniform(seed, 0.5, 1.5, *shape) * torch.sign(randn(seed + 1, *shape) + 1e-6)).contiguous()
    v = randn(seed, *shape)
    if cls == "wide":
        flat = v.reshape(-1)
        far = torch.tensor([100.0, -100.0, 88.0, -89.0, 50.0, -30.0, 17.0, -104.0])
        idx = torch.arange(0, flat.numel(), 7)
        flat[idx] = far[(idx // 7) % far.numel()]
    return v.contiguous()


def linear_inputs(cls, seed, B, K, J):
    """x [B, K] of the class, wt [K, J] (count: the class; otherwise N(0, 1)), bias [J] N(0, 1)."""
    return class_tensor(cls, seed, B, K), class_tensor("count" if cls == "count" else "normal", seed + 2, K, J), randn(seed + 4, J)


def linear64(x, wt, bias, in_act, out_act):
    a = x.double()
    v = (silu64(a) if in_act else a) @ wt.double()
    if bias is not None:
        v = v + bias.double()
    return silu64(v) if out_act else v


def linear_scale64(x, wt, bias, in_act):
    """sum_k |act(x_k) w_kj| + |bias_j| in fp64: what every per-element error is divided by."""
    a = x.double()
    s = (silu64(a) if in_act else a).abs() @ wt.double().abs()
    return s + (bias.double().abs() if bias is not None else 0.0)


def linear32_eager(x, wt, bias, in_act, out_act):
    """time_embed / emb_layers as the reference runs them: F.silu and F.linear in fp32 (weight = wt^T)."""
    v = F.linear(F.silu(x) if in_act else x, wt.t().contiguous(), bias)
    return F.silu(v) if out_act else v


def _silu32_np(v):
    with np.errstate(over="ignore"):
        return (v / (np.float32(1) + np.exp(-v, dtype=np.float32))).astype(np.float32)


def linear32_kernel_order(x, wt, bias, in_act, out_act, form):
    """The kernels' summation order in fp32 (numpy): form 0 an fmaf chain per block of 32 k, the blocks added up in order; form 1 four chains
    over the quarters of K, merged left to right; then the bias.  (One chain over all of K, as the slab kernel summed before this test
    existed, gives 1.12 x the budget at K = 2048 here.)"""
    xa, w = x.numpy().astype(np.float32), wt.numpy().astype(np.float32)
    if in_act:
        xa = _silu32_np(xa)
    K = xa.shape[1]
    bounds = [(k, min(k + 32, K)) for k in range(0, K, 32)] if form == 0 else [(q * (K // 4), (q + 1) * (K // 4)) for q in range(4)]
    parts = []
    for lo, hi in bounds:
        acc = np.zeros((xa.shape[0], w.shape[1]), dtype=np.float32)
        for k in range(lo, hi):   # fmaf: the product of two fp32 numbers is exact in fp64, the sum is rounded to fp32 (after one fp64 rounding far below it)
            acc = (acc.astype(np.float64) + xa[:, k:k + 1].astype(np.float64) * w[k:k + 1, :].astype(np.float64)).astype(np.float32)
        parts.append(acc)
    v = parts[0]
    for p in parts[1:]:
        v = v + p
    if bias is not None:
        v = v + bias.numpy().astype(np.float32)
    return torch.from_numpy(_silu32_np(v) if out_act else v)


def linear_form(B, K):
    """linear_form of csrc/embed.hip: 1 = the K-split small kernel, 0 = the slab kernel."""
    return 1 if B <= 8 and K % 32 == 0 else 0


# (B, K, J): each extreme of B, K and J with the others varied, not the cube
LINEAR_CASES = (
    # the small kernel: B in 1, 3, 8; K in 32, 96, 512, 4096 (no limit on K); J in 1, 63, 64, 65, 200 (64 outputs per workgroup)
    [(1, 32, 1), (1, 32, 63), (1, 32, 64), (1, 32, 65), (1, 32, 200), (3, 32, 64), (8, 32, 200), (1, 96, 65), (3, 96, 65), (8, 96, 65), (3, 96, 200),
     (3, 512, 64), (8, 512, 63), (1, 512, 200), (3, 4096, 64), (1, 4096, 1), (8, 4096, 200)]
    # the slab kernel reached by B > 8: B in 9, 16, 17, 300; K in 4, 36, 100, 2048; J in 1, 127, 128, 129, 640 (128 outputs per workgroup)
    + [(9, 4, 1), (9, 4, 127), (9, 4, 128), (9, 4, 129), (9, 4, 640), (300, 4, 640), (9, 36, 129), (16, 36, 129), (17, 36, 129), (300, 36, 129),
       (16, 100, 127), (17, 100, 128), (300, 100, 129), (17, 2048, 128), (9, 2048, 640), (300, 2048, 1), (16, 2048, 129)]
    # the slab kernel reached by B <= 8 with K % 32 != 0
    + [(1, 48, 1), (1, 48, 127), (1, 48, 128), (1, 48, 129), (1, 48, 640), (8, 48, 1), (8, 48, 129), (8, 48, 640)])
ACTS = ((0, 0), (1, 0), (0, 1), (1, 1))


def linear_runs(cases=LINEAR_CASES):
    """Every run of the GPU test: (tag, x, wt, bias or None, in_act, out_act, form)."""
    for ci, (B, K, J) in enumerate(cases):
        for li, cls in enumerate(LINEAR_CLASSES):
            x, wt, bias = linear_inputs(cls, 5000 + 31 * ci + 7 * li, B, K, J)
            for in_act, out_act in ACTS:
                for b in (bias, None):
                    yield (f"linear B={B} K={K} J={J} {cls} in_act={in_act} out_act={out_act} bias={b is not None}", x, wt, b, in_act, out_act,
                           linear_form(B, K))


def norm_err(got, x, wt, bias, in_act, out_act):
    """Largest normalised error of got [B, J]."""
    return float(((got.double() - linear64(x, wt, bias, in_act, out_act)).abs() / linear_scale64(x, wt, bias, in_act)).max())


# ---- the class-conditional linear -----------------------------------------------------------------------------------------------------------
def label_rows64(h, h_div, lemb, labels, n_classes, R, label_after_silu=False, mod_rows=False):
    """The staged rows silu(h[r / h_div] + lemb[lab(r)]) [R, K] in fp64; a label out of range adds nothing.  The two flags are mutants."""
    r = torch.arange(R)
    lab = labels.long() if labels is not None else r % n_classes
    ok = (lab >= 0) & (lab < n_classes)
    le = torch.where(ok[:, None], lemb.double()[lab.clamp(0, n_classes - 1)], torch.zeros((), dtype=torch.float64))
    hr = h.double()[((r % h_div) % h.shape[0]) if mod_rows else r // h_div]
    return silu64(hr) + le if label_after_silu else silu64(hr + le)


def label_linear64(h, h_div, lemb, labels, n_classes, wt, bias, R):
    v = label_rows64(h, h_div, lemb, labels, n_classes, R) @ wt.double()
    return v + bias.double() if bias is not None else v


def label_scale64(h, h_div, lemb, labels, n_classes, wt, bias, R):
    s = label_rows64(h, h_div, lemb, labels, n_classes, R).abs() @ wt.double().abs()
    return s + (bias.double().abs() if bias is not None else 0.0)


def label_linear32_eager(h, h_div, lemb, labels, n_classes, wt, bias, R):
    """emb = time_embed(.) + label_emb(y), then emb_layers, in fp32 as the reference runs them (valid labels)."""
    r = torch.arange(R)
    lab = labels.long() if labels is not None else r % n_classes
    return F.linear(F.silu(h[r // h_div] + F.embedding(lab, lemb)), wt.t().contiguous(), bias)


def label_form(K):
    """label_emb_linear_form of csrc/embed.hip: rows per slab."""
    return 16 if 16 * K * 4 <= 64 * 1024 else 8


# (R, K, J, n_classes): R in 1, 15, 16, 17, 33; K across the 16-row / 8-row boundary 1024 | 1028; J in 127, 129, 640; n_classes in 1, 7, 10
LABEL_CASES = [(1, 128, 127, 1), (15, 128, 129, 7), (16, 128, 640, 10), (17, 128, 127, 7), (33, 128, 129, 10), (33, 128, 640, 1),
               (1, 1024, 129, 7), (16, 1024, 127, 10), (17, 1024, 640, 7), (33, 1024, 129, 10),
               (1, 1028, 127, 10), (15, 1028, 129, 1), (17, 1028, 127, 7), (33, 1028, 640, 10),
               (16, 2048, 129, 7), (17, 2048, 127, 10), (33, 2048, 129, 1), (15, 2048, 640, 7)]
MAPPINGS = ("per_image", "shared", "table")


def label_inputs(ci, mi, cls, R, K, J, ncls):
    """-> dict(h, h_div, lemb, labels or None, wt, bias) for mapping MAPPINGS[mi].  per_image: a time row per output row; shared: one time row;
    table: labels None, h_div = n_classes, row r = (step r / n_classes, class r % n_classes)."""
    seed = 7000 + 53 * ci + 11 * mi + 3 * LINEAR_CLASSES.index(cls)
    mapping = MAPPINGS[mi]
    h_div = {"per_image": 1, "shared": R, "table": ncls}[mapping]
    rows_h = (R - 1) // h_div + 1
    wt = class_tensor("count" if cls == "count" else "normal", seed + 2, K, J)
    labels = None if mapping == "table" else torch.from_numpy(np.random.RandomState(seed + 5).randint(0, ncls, size=R).astype(np.int32))
    return dict(h=class_tensor(cls, seed, rows_h, K), h_div=h_div, lemb=class_tensor(cls, seed + 7, ncls, K), labels=labels, wt=wt, bias=randn(seed + 4, J))


def label_runs(cases=LABEL_CASES):
    """Every run of the GPU test: (tag, inputs, R, n_classes, form)."""
    for ci, (R, K, J, ncls) in enumerate(cases):
        for mi, mapping in enumerate(MAPPINGS):
            cls = LINEAR_CLASSES[(ci + mi) % 3]
            yield f"label linear R={R} K={K} J={J} classes={ncls} {mapping} {cls}", label_inputs(ci, mi, cls, R, K, J, ncls), R, ncls, label_form(K)


def label_norm_err(got, d, R, ncls):
    args = (d["h"], d["h_div"], d["lemb"], d["labels"], ncls, d["wt"], d["bias"], R)
    return float(((got.double() - label_linear64(*args)).abs() / label_scale64(*args)).max())


@functools.lru_cache(maxsize=None)
def linear_eager_errors():
    """K -> the largest normalised error of the fp32 eager restatement over every run with that K (both linear ops)."""
    worst = {}
    for _, x, wt, b, ia, oa, _ in linear_runs():
        K = x.shape[1]
        worst[K] = max(worst.get(K, 0.0), norm_err(linear32_eager(x, wt, b, ia, oa), x, wt, b, ia, oa))
    for _, d, R, ncls, _ in label_runs():
        K = d["h"].shape[1]
        got = label_linear32_eager(d["h"], d["h_div"], d["lemb"], d["labels"], ncls, d["wt"], d["bias"], R)
        worst[K] = max(worst.get(K, 0.0), label_norm_err(got, d, R, ncls))
    return worst


def linear_budget(K):
    return 4.0 * linear_eager_errors()[K]


# ---- pack / unpack / resample ---------------------------------------------------------------------------------------------------------------
# exact ties of bf16 (8 significand bits) and fp16 (11), +-0, beyond fp16's 65504 (65520 is the tie that rounds to inf), fp16 subnormals and their ties
SPECIALS = [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -8), 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 3 * 2.0 ** -11),
            1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -8 - 2.0 ** -20, 1.0 + 2.0 ** -11 + 2.0 ** -23, 1.0 + 2.0 ** -11 - 2.0 ** -23,
            0.0, -0.0, 65504.0, 65519.0, 65520.0, 65536.0, -70000.0, 1e5, -3e38, 3.4e38, 255.5, 1023.5, -2047.0, 2049.0,
            2.0 ** -24, 2.0 ** -25, -(2.0 ** -25), 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 2.0 ** -25 * 1.0000001, 3e-8, -6e-8, 1e-7, 6.1e-5, 6.0975e-5, 2.0 ** -14 - 2.0 ** -26]


def with_specials(x, ci):
    """Every other element of x replaced by the special values in turn (rotated by the case index)."""
    sp = torch.tensor(SPECIALS, dtype=torch.float32)
    flat = x.reshape(-1)
    idx = torch.arange(0, flat.numel(), 2)
    flat[idx] = sp[(idx // 2 + 5 * ci) % sp.numel()]
    return x


def pack_ref(x, cond, cpad, tdtype):
    """cat(x, cond, zeros) in NHWC [B, HW, cpad], cast by torch (round to nearest even)."""
    B, hw = x.shape[0], x[0, 0].numel()
    parts = [x.reshape(B, x.shape[1], hw)] + ([cond.reshape(B, cond.shape[1], hw)] if cond is not None else [])
    c = sum(p.shape[1] for p in parts)
    full = torch.cat(parts + [torch.zeros(B, cpad - c, hw)], dim=1)
    return full.permute(0, 2, 1).contiguous().to(tdtype)


def pack_truncating(x, cond, cpad, tdtype):
    """Mutant: the two-byte cast drops the low bits (bf16: the low half of the fp32 word; fp16: toward zero)."""
    full = pack_ref(x, cond, cpad, torch.float32)
    if tdtype == torch.bfloat16:
        return (full.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)
    r = full.to(tdtype)
    over = r.float().abs() > full.abs()
    return torch.where(over, torch.nextafter(r, torch.zeros_like(r)), r)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


PACK_CHANNELS = [(1, 0), (3, 0), (3, 3), (1, 1), (4, 3), (8, 0), (5, 6)]


def pack_cases(tdtype):
    """(case index, B, HW, Cx, Cc, cpad): every channel split at the next multiple of the fragment and at 32, over N in 1, 3 and HW in 1, 49, 784."""
    V = 4 if tdtype == torch.float32 else 8
    out = []
    for (cx, cc) in PACK_CHANNELS:
        for cpad in ((cx + cc + V - 1) // V * V, 32):
            B, hw = ((1, 1), (3, 49), (1, 784), (3, 1), (1, 49), (3, 784))[len(out) % 6]
            out.append((len(out), B, hw, cx, cc, cpad))
    return out


def pack_inputs(ci, B, hw, cx, cc):
    x = with_specials(randn(8000 + ci, B, cx, hw), ci)
    cond = with_specials(randn(8100 + ci, B, cc, hw), ci + 3) if cc else None
    return x, cond


def pool_tolerance(x64, ref, tdtype):
    """u_T |ref| + 3 u32 mean |in| per output element; x64 NCHW."""
    return U_STORE[tdtype] * ref.abs() + 3 * U32 * F.avg_pool2d(x64.abs(), 2)


def pool_pair_rounded(x, tdtype):
    """Mutant: each horizontal pair is rounded to the element type before the pairs are summed (x NCHW fp32 holding values of the type)."""
    H, W = x.shape[2] // 2 * 2, x.shape[3] // 2 * 2
    v = x[:, :, :H, :W]
    pair = (v[:, :, :, 0::2] + v[:, :, :, 1::2]).to(tdtype).float()
    return (0.25 * (pair[:, :, 0::2] + pair[:, :, 1::2])).to(tdtype)


POOL_SIZES = [(2, 2), (7, 7), (8, 6), (28, 28)]
POOL_CHANNELS = (1, 8, 40)


def resample_cases():
    """(case index, N, C, Hs, Ws): every size with every channel count, N alternating 1, 3."""
    out = []
    for (hs, ws) in POOL_SIZES:
        for c in POOL_CHANNELS:
            out.append((len(out), (1, 3)[len(out) % 2], c, hs, ws))
    return out


def resample_input(ci, N, C, Hs, Ws, tdtype):
    """NCHW fp32 values of the element type: noise with an offset so that pooled sums do not cancel to nothing everywhere."""
    return (randn(9000 + ci, N, C, Hs, Ws) * 1.5 + 0.25).to(tdtype).float()


# ==== the tests ============================================================================================================================
def test_references_are_the_oracle():
    t = torch.tensor([0.0, 0.5, 3.0, 250.0, 999.0])
    for dim in (32, 33, 128):
        torch.testing.assert_close(timestep_embedding64(t, dim).float(), unet_ref.timestep_embedding(t, dim), rtol=0, atol=2e-4)
        torch.testing.assert_close(timestep_embedding32_eager(t, dim), unet_ref.timestep_embedding(t, dim), rtol=0, atol=0)
    # time_embed as torch modules in fp64 = two calls of linear64
    lin0, lin1 = torch.nn.Linear(32, 128).double(), torch.nn.Linear(128, 128).double()
    x = randn(1, 5, 32)
    want = lin1(F.silu(lin0(x.double())))
    h = linear64(x, lin0.weight.detach().t().float().double(), lin0.bias.detach(), 0, 1)
    got = linear64(h, lin1.weight.detach().t(), lin1.bias.detach(), 0, 0)
    torch.testing.assert_close(got, want.detach(), rtol=1e-12, atol=1e-12)
    # emb_layers over emb + label_emb(y) = the label linear, in all three mappings
    for _, d, R, ncls, _ in label_runs(LABEL_CASES[:3]):
        r = torch.arange(R)
        lab = d["labels"].long() if d["labels"] is not None else r % ncls
        emb = d["h"].double()[r // d["h_div"]] + d["lemb"].double()[lab]
        want = F.linear(F.silu(emb), d["wt"].double().t(), d["bias"].double())
        torch.testing.assert_close(label_linear64(d["h"], d["h_div"], d["lemb"], d["labels"], ncls, d["wt"], d["bias"], R), want, rtol=1e-12, atol=1e-12)


def test_case_lists_reach_both_forms_of_both_linears():
    forms = {(linear_form(B, K), "small" if B <= 8 else "big") for B, K, _ in LINEAR_CASES}
    assert forms == {(1, "small"), (0, "big"), (0, "small")}
    assert {label_form(K) for _, K, _, _ in LABEL_CASES} == {16, 8}
    assert label_form(1024) == 16 and label_form(1028) == 8
    for vals, col in (((1, 3, 8, 9, 16, 17, 300), 0), ((32, 96, 512, 4096, 4, 36, 100, 2048, 48), 1), ((1, 63, 64, 65, 200, 127, 128, 129, 640), 2)):
        assert {c[col] for c in LINEAR_CASES} == set(vals)
    assert {c[0] for c in LABEL_CASES} == {1, 15, 16, 17, 33} and {c[1] for c in LABEL_CASES} == {128, 1024, 1028, 2048}
    assert {c[2] for c in LABEL_CASES} == {127, 129, 640} and {c[3] for c in LABEL_CASES} == {1, 7, 10}
    cls = torch.cat([t_class(t) for _, t, _, _ in timestep_cases()])
    assert set(cls.tolist()) == {0, 1, 2, 3}
    every = torch.cat([t for _, t, _, _ in timestep_cases()])
    for v in (0.0, 999.0, 1e4, -3.0, 0.5):
        assert bool((every == v).any()), v


def test_linear_budgets_and_the_kernels_summation_order():
    """(ii) the eager restatement is inside the budget by construction; the kernels' own summation order in fp32 is inside it too."""
    errs = linear_eager_errors()
    print("   EMBREF linear e_ref per K: " + " ".join(f"{K}: {errs[K]:.1e}" for K in sorted(errs)))
    assert all(0 < e < 1e-6 for e in errs.values()), errs
    worst = 0.0
    for ci, (tag, x, wt, b, ia, oa, form) in enumerate(linear_runs()):
        if ci % 5:      # every fifth run: every case, class and setting is met over the list
            continue
        e = norm_err(linear32_kernel_order(x, wt, b, ia, oa, form), x, wt, b, ia, oa)
        worst = max(worst, e / linear_budget(x.shape[1]))
        assert e <= linear_budget(x.shape[1]), f"{tag}: the kernel's summation order in fp32 gives {e:.3e} > budget {linear_budget(x.shape[1]):.3e}"
    print(f"   EMBREF linear, kernel order in fp32: worst error / budget {worst:.2f}")


def _count_case(B, K, J, seed=123):
    return linear_inputs("count", seed + B + K + J, B, K, J)


def test_linear_mutants_break_the_budget():
    """(iii) on "every term counts" inputs one missing or misplaced term is orders of magnitude above the budget."""
    for (B, K, J) in [(1, 32, 65), (3, 4096, 64), (9, 4, 129), (17, 2048, 128), (1, 48, 127), (300, 100, 129)]:
        x, wt, bias = _count_case(B, K, J)
        bud = linear_budget(K)
        for ia, oa in ACTS:
            a = silu64(x.double()) if ia else x.double()
            full = a @ wt.double() + bias.double()
            fin = (lambda v: silu64(v)) if oa else (lambda v: v)
            muts = {"drops the last k": fin(full - a[:, -1:] @ wt.double()[-1:]), "takes bias[j - 1]": fin(full - bias.double() + bias.double().roll(1))}
            if K % 32:
                keep = K // 32 * 32
                muts["drops the tail beyond a multiple of 32"] = fin(a[:, :keep] @ wt.double()[:keep] + bias.double())
            if linear_form(B, K) == 1:
                q = K // 4
                muts["skips the second wave's quarter of K"] = fin(full - a[:, q:2 * q] @ wt.double()[q:2 * q])
            if B >= 8:
                z = fin(full).clone()
                z[7::8] = 0.0
                muts["leaves the last row of a slab at zero"] = z
            for name, got in muts.items():
                if name == "takes bias[j - 1]" and J == 1:
                    continue
                e = norm_err(got, x, wt, bias, ia, oa)
                assert e > 100 * bud, f"B={B} K={K} J={J} acts={ia}{oa}: a linear that {name} errs by {e:.3e}, budget {bud:.3e}: the test could not see it"
        # one of the two SiLUs omitted
        for got in (linear64(x, wt, bias, 0, 1), linear64(x, wt, bias, 1, 0)):
            assert norm_err(got, x, wt, bias, 1, 1) > 100 * bud
    # a tail beyond a multiple of 4: no K the launchers accept has one, so the mutant is shown on K = 38 against that K's own eager error
    x, wt, bias = _count_case(9, 38, 65)
    e_ref = norm_err(linear32_eager(x, wt, bias, 0, 0), x, wt, bias, 0, 0)
    got = x.double()[:, :36] @ wt.double()[:36] + bias.double()
    assert norm_err(got, x, wt, bias, 0, 0) > 100 * 4 * e_ref


def test_label_linear_mutants_break_the_budget():
    seen = set()
    for tag, d, R, ncls, _ in label_runs():
        K = d["h"].shape[1]
        args = (d["h"], d["h_div"], d["lemb"], d["labels"], ncls)
        ref, scale = label_linear64(*args, d["wt"], d["bias"], R), label_scale64(*args, d["wt"], d["bias"], R)
        after = label_rows64(*args, R, label_after_silu=True) @ d["wt"].double() + d["bias"].double()
        assert float(((after - ref).abs() / scale).max()) > 100 * linear_budget(K), f"{tag}: the label row added after the SiLU is not seen"
        if d["h"].shape[0] > 1:      # more than one time row: r % h_div picks another one somewhere
            mod = label_rows64(*args, R, mod_rows=True) @ d["wt"].double() + d["bias"].double()
            assert float(((mod - ref).abs() / scale).max()) > 100 * linear_budget(K), f"{tag}: r % h_div for r / h_div is not seen"
            seen.add(tag.split()[-2])
    assert seen == {"per_image", "table"}, seen


def test_timestep_budgets_and_mutants():
    errs = timestep_eager_errors()
    print("   EMBREF timestep e_ref per class: " + " ".join(f"{c}: {e:.1e}" for c, e in zip(T_CLASSES, errs)))
    assert all(e > 0 for e in errs) and errs[0] < 1e-6 and errs[3] < 1e-2, errs
    seen = {"swap": [False] * 4, "half": [False] * 4}
    for ci, t, dim, mp in timestep_cases():
        check_timestep(timestep_embedding32_eager(t, dim, mp), t, dim, mp, f"eager dim={dim} B={t.numel()} mp={mp}")
        half = dim // 2
        want = timestep_embedding64(t, dim, mp)
        swapped = torch.cat([want[:, half:2 * half], want[:, :half], want[:, 2 * half:]], dim=1)
        muts = {"swap": swapped}
        if half >= 2:
            f = torch.exp(-math.log(mp) * torch.arange(half, dtype=torch.float64) / (half - 1))
            a = t.double()[:, None] * f[None]
            muts["half"] = torch.cat([torch.cos(a), torch.sin(a), want[:, 2 * half:]], dim=1)
        buds = timestep_budgets()
        for name, got in muts.items():
            e = class_errors(got, want, t)
            cls = t_class(t)
            for k in range(4):
                # a time of exactly 0 hides a wrong frequency (every argument is 0); the swap is seen there too (cos 0 = 1, sin 0 = 0)
                rows = (cls == k) & ((t != 0) | (name == "swap"))
                if bool(rows.any()):
                    assert e[k] > 10 * buds[k], f"dim={dim} B={t.numel()} mp={mp}: mutant {name} errs by {e[k]:.3e} in class {T_CLASSES[k]}, budget {buds[k]:.3e}"
                    seen[name][k] = True
    assert all(seen["swap"]) and all(seen["half"]), seen


@pytest.mark.parametrize("tdtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_pack_reference_rounds_to_nearest_even_and_truncation_is_seen(tdtype):
    one = torch.tensor(SPECIALS, dtype=torch.float32)
    r = one.to(tdtype).float()
    if tdtype == torch.bfloat16:
        assert float(r[0]) == 1.0 and float(r[1]) == 1.0 + 2.0 ** -6 and float(r[6]) == 1.0 + 2.0 ** -7 and float(r[7]) == 1.0   # ties to even; just above / below a tie
        assert math.isinf(float(torch.tensor(3.4e38).to(tdtype)))
    else:
        assert float(r[3]) == 1.0 and float(r[4]) == 1.0 + 2.0 ** -9 and float(r[8]) == 1.0 + 2.0 ** -10 and float(r[9]) == 1.0
        assert float(one[12].to(tdtype)) == 65504.0 and float(one[13].to(tdtype)) == 65504.0 and math.isinf(float(one[14].to(tdtype)))
        assert float(r[24]) == 2.0 ** -24 and float(r[25]) == 0.0 and float(r[27]) == 2.0 ** -23 and float(r[29]) == 2.0 ** -24   # subnormals: ties to even
    assert bits(torch.tensor([-0.0]).to(tdtype)).item() != 0
    differs = 0
    for ci, B, hw, cx, cc, cpad in pack_cases(tdtype):
        x, cond = pack_inputs(ci, B, hw, cx, cc)
        ref, mut = pack_ref(x, cond, cpad, tdtype), pack_truncating(x, cond, cpad, tdtype)
        assert ref.shape == (B, hw, cpad) and bool((ref[:, :, cx + cc:] == 0).all())
        if hw > 1:
            assert not torch.equal(bits(ref), bits(mut)), f"case {ci}: a truncating pack equals the rounding one: the inputs hold no value that tells them apart"
            differs += 1
    assert differs >= 8


@pytest.mark.parametrize("tdtype", [torch.float32, torch.bfloat16, torch.float16], ids=["fp32", "bf16", "fp16"])
def test_pool_tolerance_passes_one_rounding_and_sees_pair_rounding(tdtype):
    for ci, N, C, Hs, Ws in resample_cases():
        x = resample_input(ci, N, C, Hs, Ws, tdtype)
        ref = F.avg_pool2d(x.double(), 2)
        assert ref.shape[2:] == (Hs // 2, Ws // 2)
        tol = pool_tolerance(x.double(), ref, tdtype)
        v = x[:, :, :Hs // 2 * 2, :Ws // 2 * 2]
        good = (0.25 * ((v[:, :, 0::2, 0::2] + v[:, :, 0::2, 1::2]) + (v[:, :, 1::2, 0::2] + v[:, :, 1::2, 1::2]))).to(tdtype)   # the kernel's expression
        assert float(((good.double() - ref).abs() - tol).max()) <= 0, f"case {ci}: fp32 pooling with one store rounding misses the tolerance"
        if tdtype != torch.float32 and ref.numel() >= 64:
            bad = pool_pair_rounded(x, tdtype)
            assert float(((bad.double() - ref).abs() - tol).max()) > 0, f"case {ci}: rounding each pair to the element type is inside the tolerance"
