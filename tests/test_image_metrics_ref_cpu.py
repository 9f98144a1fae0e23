"""CPU: the fp64 restatement of mi355_image_metrics (tests/image_metrics_ref.py) against skimage's construction of the same numbers, its exact
properties, the entry point's argument checks through the built library (no GPU needed), and evaluation.evaluate's key order."""
import ctypes as C
import json

import pytest
import torch

from tests import image_metrics_ref as R

WINDOWS = [pytest.param(False, id="uniform7"), pytest.param(True, id="gauss11")]


def _cases(gaussian):
    return [(s, "random") for s in R.CASES if not gaussian or min(s[2:]) >= 11] + [(R.SMOOTH, "smooth")]


@pytest.mark.parametrize("gaussian", WINDOWS)
def test_restatement_agrees_with_full_image_filtering(gaussian):
    """avg_pool2d / conv2d at the valid positions against scipy.ndimage over the full image and the crop (skimage's way): two summation
    orders of the same fp64 sums, 1e-14 apart at the most on every shape of the table and on the smooth pair."""
    worst = 0.0
    for shape, kind in _cases(gaussian):
        x, ref = R.pair(shape) if kind == "random" else R.smooth_pair(shape)
        for data_range in (None, 2.0):
            a = R.want(shape, kind, gaussian, data_range)
            b = R.metrics_scipy(x, ref, data_range=data_range, gaussian=gaussian)
            for k in ("mse", "data_range", "psnr", "ssim"):
                worst = max(worst, (a[k] - b[k]).abs().max().item())
    print(f"two fp64 constructions: max |difference| = {worst:.3e}")
    assert worst <= 1e-14


@pytest.mark.parametrize("gaussian", WINDOWS)
def test_identical_images_score_exactly_one_and_infinity(gaussian):
    for shape, kind in _cases(gaussian):
        x, _ = R.pair(shape) if kind == "random" else R.smooth_pair(shape)
        for data_range in (None, 2.0):
            m = R.metrics_ref(x, x, data_range=data_range, gaussian=gaussian)
            assert m["ssim"].tolist() == [1.0] * shape[0], (shape, kind, data_range)
            assert m["psnr"].tolist() == [float("inf")] * shape[0], (shape, kind, data_range)
            assert m["mse"].tolist() == [0.0] * shape[0]


def test_window_defaults():
    taps, win, cov = R.window(True)
    assert win == 11 and cov == 1.0 and taps.dtype == torch.float32 and abs(taps.double().sum().item() - 1.0) < 1e-7
    assert torch.equal(taps, taps.flip(0)) and taps.argmax().item() == 5
    assert R.window(False)[1:] == (7, float(torch.tensor(49.0 / 48.0, dtype=torch.float32)))
    assert R.window(False, use_sample_covariance=False)[2] == 1.0


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as ge

    ge.build()


def _call(**over):
    """mi355_image_metrics with valid host-side arguments except for `over`; the pointers are never dereferenced before the checks."""
    from mi355 import _lib

    a = dict(x=C.c_void_p(256), ref=C.c_void_p(512), out=C.c_void_p(768), batch=2, channels=3, h=16, w=16, data_range=0.0, taps=None, win=7,
             cov_norm=49.0 / 48.0, k1=0.01, k2=0.03)
    a.update(over)
    L = _lib.lib()
    rc = L.mi355_image_metrics(a["x"], a["ref"], a["out"], a["batch"], a["channels"], a["h"], a["w"], a["data_range"], a["taps"], a["win"],
                               a["cov_norm"], a["k1"], a["k2"], None)
    return rc, L.mi355_last_error().decode()


@pytest.mark.parametrize("name,over", [
    ("x", dict(x=None)), ("ref", dict(ref=None)), ("out", dict(out=None)),
    ("batch", dict(batch=0)), ("channels", dict(channels=0)), ("h", dict(h=0)), ("w", dict(w=-3)),
    ("win", dict(win=4)), ("win", dict(win=1)), ("win", dict(win=17)), ("win", dict(win=7, h=5, w=9)), ("win", dict(win=11, h=32, w=10)),
    ("k1", dict(k1=-0.01)), ("k2", dict(k2=-1.0)), ("cov_norm", dict(cov_norm=0.0)), ("cov_norm", dict(cov_norm=-1.0)),
    ("h", dict(h=4097)), ("w", dict(w=4097)),
])
def test_bad_arguments_are_refused_on_the_host(built, name, over):
    """Every refusal of include/mi355_sampler.h answers before any device call - on a machine without a GPU too - with MI355_ERR_ARG and a
    message that names the argument."""
    rc, msg = _call(**over)
    assert rc == -1, (rc, msg)
    assert msg.startswith(f"image_metrics: {name} "), msg


class _StubOps:
    """image_metrics / mse_per_sample computed by the restatement on the CPU; counts the calls."""

    def __init__(self):
        self.calls = []

    def image_metrics(self, x, ref):
        self.calls.append("image_metrics")
        return {k: v.float() for k, v in R.metrics_ref(x, ref).items()}

    def mse_per_sample(self, a, b):
        self.calls.append("mse_per_sample")
        return R.metrics_ref(a, b)["mse"].float()


class _Identity:
    def sample(self, batch):
        return batch


def test_evaluate_key_order_and_one_call_per_batch(tmp_path, monkeypatch):
    import evaluation

    batches = [R.pair((3, 1, 16, 16), seed=k)[1] for k in range(2)]
    samples = iter([R.pair((3, 1, 16, 16), seed=k)[0] for k in range(2)])
    stub = _StubOps()
    monkeypatch.setattr(evaluation, "default_ops", stub)
    res = evaluation.evaluate(lambda xT, cond: next(samples), _Identity(), batches, tmp_path, save_images=False,
                              metrics=("mse", "lpips", "psnr", "ssim"))
    assert list(res.keys()) == ["mse_mean", "lpips_mean", "psnr_mean", "ssim_mean", "mse_median", "lpips_median", "psnr_median", "ssim_median",
                                "mse_std", "lpips_std", "psnr_std", "ssim_std", "fid"]
    assert stub.calls == ["image_metrics", "image_metrics"]          # one launch per batch, the MSE from the same call
    assert json.load(open(tmp_path / "results.json")) == res
    every = {k: torch.cat([R.metrics_ref(R.pair((3, 1, 16, 16), seed=s)[0], b)[k].float() for s, b in enumerate(batches)]) for k in ("mse", "psnr", "ssim")}
    for k, v in every.items():
        assert res[f"{k}_mean"] == v.mean().item() and res[f"{k}_median"] == v.median().item() and res[f"{k}_std"] == v.std().item()
    assert res["lpips_mean"] is None and res["fid"] is None

    # the default is what it was: the two reference keys, the MSE op alone
    samples = iter([R.pair((3, 1, 16, 16), seed=k)[0] for k in range(2)])
    stub.calls.clear()
    res2 = evaluation.evaluate(lambda xT, cond: next(samples), _Identity(), batches, tmp_path, save_images=False)
    assert list(res2.keys()) == ["mse_mean", "lpips_mean", "mse_median", "lpips_median", "mse_std", "lpips_std", "fid"]
    assert stub.calls == ["mse_per_sample", "mse_per_sample"]
    assert all(res2[k] == res[k] for k in res2)

    with pytest.raises(ValueError, match="unknown metrics"):
        evaluation.evaluate(lambda xT, cond: xT, _Identity(), batches, tmp_path, save_images=False, metrics=("mse", "fsim"))
