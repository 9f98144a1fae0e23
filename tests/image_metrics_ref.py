"""Per-sample MSE, data range, PSNR and SSIM of an image batch against its ground truth in fp64, two ways, and the case table of their tests.

  metrics_ref     what csrc/metrics.hip computes (include/mi355_sampler.h, mi355_image_metrics), in plain torch on the CPU: the difference in
                  fp32, everything after it in fp64; window means at the positions wholly inside the image from F.avg_pool2d (uniform window)
                  or two F.conv2d passes, rows then columns, with the fp32 taps widened to double (Gaussian window), no padding
  metrics_scipy   the way skimage.metrics.structural_similarity computes the same numbers: scipy.ndimage.uniform_filter / correlate1d over
                  the FULL image, then the crop of (win - 1) / 2 pixels (the border mode never reaches the cropped interior)
  CASES           the shapes tests/test_gpu_image_metrics.py runs; tests/test_image_metrics_ref_cpu.py holds the two constructions together

skimage's defaults: a uniform 7 x 7 window with the sample covariance (cov_norm = 49 / 48), or Gaussian weights of sigma 1.5 truncated at 3.5 sigma
(11 taps, cov_norm = 1); K1 = 0.01, K2 = 0.03; data_range None = max(ref) - min(ref) of each sample (AD/image_diffusion/trainer2.py:15-30).
k1, k2 and cov_norm cross the C ABI as fp32, so they are rounded to fp32 here as well.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from mi355.synth import rand_uniform, randn

# [B, C, H, W]; the kernel's tile is 16 window rows x 32 window columns
CASES = [
    (3, 1, 7, 7),       # a single window position
    (2, 3, 8, 7),       # non-square, one position along one axis
    (3, 1, 28, 28),     # MNIST
    (2, 3, 32, 32),     # CIFAR
    (2, 2, 19, 13),     # odd sizes, a channel count that is not 1 or 3
    (1, 3, 64, 64),     # larger square case
    (1, 1, 150, 130),   # more rows than one band, more columns than one tile
    (1, 1, 9, 300),     # ten column tiles
    (1, 1, 300, 9),     # nineteen row bands
    (5, 3, 16, 16),     # B larger than the others, samples with different ranges
]
SMOOTH = (2, 3, 32, 32)   # the shape of the smooth pair
TOL_REL, TOL_ABS = 4 * 2.0 ** -24, 1e-6


def window(gaussian, sigma=1.5, win_size=7, use_sample_covariance=True):
    """-> (taps: float32 [win] or None for the uniform window, win, cov_norm)"""
    if gaussian:
        r = int(3.5 * sigma + 0.5)
        w = torch.exp(-0.5 * torch.arange(-r, r + 1, dtype=torch.float64) ** 2 / sigma ** 2)
        return (w / w.sum()).float(), 2 * r + 1, 1.0
    n = win_size * win_size
    return None, win_size, float(np.float32(n / (n - 1.0))) if use_sample_covariance else 1.0


@functools.lru_cache(maxsize=None)
def pair(shape, seed=0):
    """ref = rand * 2 - 1, x = clamp(ref + 0.3 * randn, -1, 1) (every sample has its own max - min, a little under 2)"""
    ref = rand_uniform(1000 + seed, -1.0, 1.0, *shape)
    x = (ref + 0.3 * randn(2000 + seed, *shape)).clamp(-1, 1)
    return x.contiguous(), ref.contiguous()


@functools.lru_cache(maxsize=None)
def smooth_pair(shape=SMOOTH, seed=0):
    """A horizontal ramp and the ramp plus 1e-3 noise: window variances of 1e-2 and less under squared means of up to 0.9 (the cancellation
    in uxx - ux * ux that costs an fp32 evaluation 8.5e-7 relative)."""
    W = shape[-1]
    ref = (0.9 * torch.linspace(-1, 1, W, dtype=torch.float32) + 0.05).expand(shape).contiguous()
    x = (ref + 1e-3 * randn(3000 + seed, *shape)).contiguous()
    return x, ref


def _finish(x, ref, data_range, means, cov_norm, K1, K2):
    """means(a: float64 [B, C, H, W]) -> the window means at the valid positions, float64 [B, C, H - win + 1, W - win + 1]"""
    d = x - ref                                                            # fp32, as the kernel forms it
    mse = (d.double() ** 2).mean(dim=(1, 2, 3))
    if data_range is None:
        R = ref.amax(dim=(1, 2, 3)).double() - ref.amin(dim=(1, 2, 3)).double()
    else:
        R = torch.full((x.shape[0],), float(data_range), dtype=torch.float64)
    psnr = 10.0 * torch.log10(R * R / mse)
    k1, k2 = float(np.float32(K1)), float(np.float32(K2))
    C1, C2 = ((k1 * R) ** 2).view(-1, 1, 1, 1), ((k2 * R) ** 2).view(-1, 1, 1, 1)
    X, Y = x.double(), ref.double()
    ux, uy, uxx, uyy, uxy = means(X), means(Y), means(X * X), means(Y * Y), means(X * Y)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return {"mse": mse, "data_range": R, "psnr": psnr, "ssim": S.mean(dim=(1, 2, 3))}


def metrics_ref(x, ref, data_range=None, gaussian=False, sigma=1.5, win_size=7, use_sample_covariance=True, K1=0.01, K2=0.03):
    """x, ref: float32 [B, C, H, W] on the CPU -> {"mse", "data_range", "psnr", "ssim"}: float64 [B]"""
    taps, win, cov_norm = window(gaussian, sigma, win_size, use_sample_covariance)
    B, C, H, W = x.shape

    def means(a):
        if taps is None:
            return F.avg_pool2d(a, win, stride=1)
        t = taps.double()
        a = F.conv2d(a.reshape(B * C, 1, H, W), t.view(1, 1, 1, win))      # rows: the horizontal pass
        return F.conv2d(a, t.view(1, 1, win, 1)).reshape(B, C, H - win + 1, W - win + 1)

    return _finish(x, ref, data_range, means, cov_norm, K1, K2)


def metrics_scipy(x, ref, data_range=None, gaussian=False, sigma=1.5, win_size=7, use_sample_covariance=True, K1=0.01, K2=0.03):
    """The same numbers with skimage's construction: filter the full image, crop the border."""
    from scipy import ndimage

    taps, win, cov_norm = window(gaussian, sigma, win_size, use_sample_covariance)
    pad = (win - 1) // 2

    def means(a):
        a = a.numpy()
        if taps is None:
            f = ndimage.uniform_filter(a, size=(1, 1, win, win))
        else:
            t = taps.double().numpy()
            f = ndimage.correlate1d(ndimage.correlate1d(a, t, axis=3), t, axis=2)
        return torch.from_numpy(np.ascontiguousarray(f[:, :, pad:f.shape[2] - pad, pad:f.shape[3] - pad]))

    return _finish(x, ref, data_range, means, cov_norm, K1, K2)


@functools.lru_cache(maxsize=None)
def want(shape, kind, gaussian, data_range):
    """The restatement for one case of the table (kind: "random" or "smooth"), computed once per session."""
    x, ref = pair(shape) if kind == "random" else smooth_pair(shape)
    return metrics_ref(x, ref, data_range=data_range, gaussian=gaussian)


def bound_ratio(got, wanted):
    """max over the entries of |got - want| / (4 * 2^-24 * |want| + 1e-6); got: float32 [B], wanted: float64 [B], both finite"""
    got, wanted = got.double().cpu(), wanted.double()
    assert torch.isfinite(got).all() and torch.isfinite(wanted).all(), (got, wanted)
    return ((got - wanted).abs() / (TOL_REL * wanted.abs() + TOL_ABS)).max().item()
