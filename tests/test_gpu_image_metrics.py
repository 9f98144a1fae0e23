"""GPU: mi355_image_metrics (csrc/metrics.hip: per-sample MSE, data range, PSNR and SSIM from one launch) against its fp64 restatement
(tests/image_metrics_ref.py), its exact properties, and the evaluation loop that reports it.

Tolerance, for each of the four outputs: |got - want| <= 4 * 2^-24 * |want| + 1e-6.  The kernel's arithmetic is fp64 on exactly representable
inputs (a product of two fp32 values is exact in fp64); it differs from the restatement by the order of the sums (1e-15) and the device's fp64
log10, and every result is rounded to fp32 once: 2^-24 relative, with a fourfold margin.  The absolute term covers a PSNR near 0 dB.
"""
import pytest
import torch

from mi355 import _lib
from tests import image_metrics_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("mse", "data_range", "psnr", "ssim")
WINDOWS = [pytest.param(False, id="uniform7"), pytest.param(True, id="gauss11")]
# every shape with the uniform 7 x 7 window, and with the 11-tap Gaussian one where it fits
TABLE = [pytest.param(s, kind, g, id=("smooth" if kind == "smooth" else "x".join(map(str, s))) + ("-gauss11" if g else "-uniform7"))
         for g in (False, True) for s, kind in [(s, "random") for s in R.CASES] + [(R.SMOOTH, "smooth")] if not g or min(s[2:]) >= 11]
_worst = {"ratio": 0.0}


@pytest.fixture(scope="module")
def ops():
    from mi355.ops import default_ops

    return default_ops


def _pair(shape, kind):
    x, ref = R.pair(shape) if kind == "random" else R.smooth_pair(shape)
    return x.to(DEV), ref.to(DEV)


def _bits(m):
    return torch.stack([m[k] for k in KEYS]).cpu().view(torch.int32)


@pytest.mark.parametrize("shape,kind,gaussian", TABLE)
def test_against_fp64_restatement(ops, shape, kind, gaussian):
    x, ref = _pair(shape, kind)
    for data_range in (None, 2.0):
        got = ops.image_metrics(x, ref, data_range=data_range, gaussian_weights=gaussian)
        want = R.want(shape, kind, gaussian, data_range)
        for k in KEYS:
            assert got[k].dtype == torch.float32 and tuple(got[k].shape) == (shape[0],)
            ratio = R.bound_ratio(got[k], want[k])
            _worst["ratio"] = max(_worst["ratio"], ratio)
            print(f"{shape} {kind} gaussian={gaussian} data_range={data_range} {k}: |got - want| / bound = {ratio:.3f}")
            assert ratio <= 1.0, (k, got[k].cpu().tolist(), want[k].tolist())
        # bit-equal to the MSE op, and from one call to the next
        assert torch.equal(got["mse"].view(torch.int32), ops.mse_per_sample(x, ref).view(torch.int32))
        again = ops.image_metrics(x, ref, data_range=data_range, gaussian_weights=gaussian)
        assert torch.equal(_bits(got), _bits(again))
    print(f"worst |got - want| / bound so far: {_worst['ratio']:.3f}")


@pytest.mark.parametrize("shape,kind,gaussian", TABLE)
def test_identical_images(ops, shape, kind, gaussian):
    x, _ = _pair(shape, kind)
    for data_range in (None, 2.0):
        m = ops.image_metrics(x, x.clone(), data_range=data_range, gaussian_weights=gaussian)
        assert m["ssim"].cpu().tolist() == [1.0] * shape[0]
        assert m["psnr"].cpu().tolist() == [float("inf")] * shape[0]
        assert m["mse"].cpu().tolist() == [0.0] * shape[0]


@pytest.mark.parametrize("gaussian", WINDOWS)
def test_each_sample_alone_and_unaligned_input(ops, gaussian):
    shape = (5, 3, 16, 16)
    x, ref = _pair(shape, "random")
    whole = ops.image_metrics(x, ref, gaussian_weights=gaussian)
    ranges = whole["data_range"].cpu().tolist()
    assert len(set(ranges)) == shape[0], ranges                      # the samples do have different ranges
    for n in range(shape[0]):
        one = ops.image_metrics(x[n:n + 1].contiguous(), ref[n:n + 1].contiguous(), gaussian_weights=gaussian)
        assert torch.equal(_bits(one)[:, 0], _bits(whole)[:, n]), n
    # x one float past an aligned base: any vector load has to fall back to scalar
    buf = torch.empty(x.numel() + 1, device=DEV, dtype=torch.float32)
    shifted = buf[1:].view(shape)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    assert torch.equal(_bits(ops.image_metrics(shifted, ref, gaussian_weights=gaussian)), _bits(whole))


def test_thin_wrappers_and_keywords(ops):
    x, ref = _pair((2, 3, 32, 32), "random")
    m = ops.image_metrics(x, ref)
    assert torch.equal(ops.psnr(x, ref), m["psnr"]) and torch.equal(ops.ssim(x, ref), m["ssim"])
    for kw in (dict(win_size=3), dict(win_size=11, use_sample_covariance=False), dict(gaussian_weights=True, sigma=0.8), dict(K1=0.02, K2=0.05)):
        got = ops.ssim(x, ref, **kw)
        ref_kw = {{"gaussian_weights": "gaussian"}.get(k, k): v for k, v in kw.items()}
        assert R.bound_ratio(got, R.metrics_ref(x.cpu(), ref.cpu(), **ref_kw)["ssim"]) <= 1.0, kw


def test_operand_checks(ops):
    x, ref = _pair((2, 3, 32, 32), "random")
    with pytest.raises(_lib.MI355BackendError, match="cpu"):
        ops.image_metrics(x.cpu(), ref)
    with pytest.raises(_lib.MI355BackendError, match="one shape"):
        ops.image_metrics(x, ref[:, :2].contiguous())
    with pytest.raises(_lib.MI355BackendError, match=r"\[B, C, H, W\]"):
        ops.image_metrics(x[0], ref[0])
    with pytest.raises(_lib.MI355BackendError, match="win"):
        ops.image_metrics(x, ref, win_size=8)
    with pytest.raises(_lib.MI355BackendError, match="data_range"):
        ops.image_metrics(x, ref, data_range=0.0)


def test_evaluation_loop_reports_psnr_and_ssim(tmp_path):
    """evaluation.evaluate with all four metrics on a tiny amortized in-painting sampler: psnr_* / ssim_* are the restatement of the recorded
    samples, mse_* is what the default run (the MSE op alone) reports for the same samples, bit for bit."""
    import json

    import evaluation
    from image_diffusion import sampling
    from image_diffusion.conditioning import Amortized
    from image_diffusion.likelihoods import InPainting
    from image_diffusion.sde_diffusion import DDPM
    from image_diffusion.unet import UNetModel, param_shapes
    from mi355.synth import rand_uniform, synth_state_dict
    from oracle import unet_ref

    cfg = unet_ref.UNetConfig(16, 2, 32, 1, 1, (2,), channel_mult=(1, 2), num_heads=2)
    net = UNetModel(image_size=16, in_channels=2, model_channels=32, out_channels=1, num_res_blocks=1, attention_resolutions=(2,),
                    channel_mult=(1, 2), num_heads=2, precision="fp32")
    net.load_state_dict(synth_state_dict(param_shapes(cfg), 1002))
    net.to(DEV)
    ddpm = DDPM(25)
    lik = InPainting(patch_size=4, pad_value=-2)
    fn = sampling.get_conditional_sample_fn(sampling.make_eps_model(net, ddpm), ddpm, Amortized(0.9, 0, 0.1), lik)
    seen = []

    def recording(xT, cond):
        seen.append(fn(xT, cond).clone())
        return seen[-1]

    torch.manual_seed(3)
    batches = [rand_uniform(70 + k, -1.0, 1.0, 3, 1, 16, 16).to(DEV) for k in range(2)]
    res = evaluation.evaluate(recording, lik, batches, tmp_path, save_images=False, metrics=("mse", "lpips", "psnr", "ssim"))
    assert list(res.keys()) == ["mse_mean", "lpips_mean", "psnr_mean", "ssim_mean", "mse_median", "lpips_median", "psnr_median", "ssim_median",
                                "mse_std", "lpips_std", "psnr_std", "ssim_std", "fid"]
    assert json.load(open(tmp_path / "results.json")) == res
    want = [R.metrics_ref(x0.float().cpu(), b.cpu()) for x0, b in zip(seen, batches)]
    for k in ("psnr", "ssim"):
        # the loop's statistics are torch.mean / median / std of the fp32 per-sample values; the same three of the restatement's values rounded to
        # fp32 differ from them only through the per-sample differences, each within b_i = 4 * 2^-24 * |v_i| + 1e-6: the mean by at most mean(b_i),
        # the median by at most max(b_i), the standard deviation (n - 1 = 5 in its denominator) by at most max(b_i) * sqrt(6 / 5)
        v = torch.cat([w[k] for w in want]).float()
        b = R.TOL_REL * v.abs().double() + R.TOL_ABS
        for stat, value, bound in (("mean", v.mean(), b.mean()), ("median", v.median(), b.max()), ("std", v.std(), b.max() * (6 / 5) ** 0.5)):
            print(f"{k}_{stat}: got {res[f'{k}_{stat}']!r}, want {value.item()!r}, bound {bound.item():.3e}")
            assert abs(res[f"{k}_{stat}"] - value.item()) <= bound.item(), (k, stat)
    replay = iter(seen)
    res_default = evaluation.evaluate(lambda xT, cond: next(replay), lik, batches, tmp_path / "default", save_images=False)
    assert list(res_default.keys()) == ["mse_mean", "lpips_mean", "mse_median", "lpips_median", "mse_std", "lpips_std", "fid"]
    for k in ("mse_mean", "mse_median", "mse_std"):
        assert res_default[k] == res[k], k
