"""The device noise path against independent answers: a plain numpy Philox4x32-10 (checked against the Random123 known answers)
rebuilds the `mi355_randn` stream value by value; the Philox branch of each DDPM step kernel is compared bit for bit with the same
kernel fed that stream as injected noise; `mi355_ddpm_sample` with device noise is compared bit for bit with the same call fed the
draws it documents (call k at offset k * n_al)."""
import numpy as np
import pytest
import torch

from mi355.synth import rand_uniform, randn

DEV = "cuda:0"
gpu = pytest.mark.gpu

# ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) in numpy --------------------------
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
SH = np.uint64(32)


def philox4x32(ctr, key, rounds=10):
    """ctr: uint32 array [n, 4]; key: (k0, k1) Python ints -> uint32 array [n, 4]."""
    c = [ctr[:, i].astype(np.uint64) for i in range(4)]
    k0, k1 = int(key[0]), int(key[1])
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]       # 32 x 32 -> 64 bit products
        c = [(p1 >> SH) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> SH) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack(c, axis=1).astype(np.uint32)


KAT = [  # Random123 kat_vectors, philox4x32 10 rounds: counter, key, output
    ([0, 0, 0, 0], (0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
    ([0xffffffff] * 4, (0xffffffff, 0xffffffff), [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
    ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0), [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
]


def test_cpu_philox_reproduces_the_random123_known_answers():
    for ctr, key, want in KAT:
        got = philox4x32(np.array([ctr], dtype=np.uint32), key)[0].tolist()
        assert got == want, ([hex(v) for v in got], [hex(v) for v in want])
    nine = philox4x32(np.array([KAT[0][0]], dtype=np.uint32), KAT[0][1], rounds=9)[0].tolist()
    assert nine != KAT[0][2]


def _uniform(r):
    """The kernel's uniform, in float32 like the kernel: (float32(r) + 0.5) * 2^-32, in (0, 1]."""
    return (r.astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -32)


def _box_muller(r):
    """uint32 [n, 4] -> float64 [n, 4]: (u0, u1) -> r cos, r sin; (u2, u3) -> r cos, r sin; fp64 from the float32 uniforms."""
    u = _uniform(r)
    assert u.dtype == np.float32
    u = u.astype(np.float64)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    ta, tb = 2.0 * np.pi * u[:, 1], 2.0 * np.pi * u[:, 3]
    return np.stack([ra * np.cos(ta), ra * np.sin(ta), rb * np.cos(tb), rb * np.sin(tb)], axis=1)


def reference_randn(seed, offset, n):
    """Elements offset .. offset + n of the stream: element e is lane e % 4 of counter (e / 4 as (lo, hi, 0, 0)), key (seed lo, seed hi)."""
    assert offset % 4 == 0
    cnt = (n + 3) // 4
    idx = offset // 4 + np.arange(cnt, dtype=np.uint64)
    ctr = np.zeros((cnt, 4), dtype=np.uint32)
    ctr[:, 0] = (idx & MASK).astype(np.uint32)
    ctr[:, 1] = (idx >> SH).astype(np.uint32)
    r = philox4x32(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    return _box_muller(r).reshape(-1)[:n]


def test_extreme_words_give_finite_normals():
    """r = 0 and r = 2^32 - 1 cannot be placed in the device stream; the formula itself: u = 2^-33 (the largest radius, 6.76) and u = 1
    (float32(2^32 - 1) + 0.5 rounds to 2^32: radius 0), both finite."""
    r = np.array([[0, 0, 0xFFFFFFFF, 0xFFFFFFFF], [0xFFFFFFFF, 0, 0, 0xFFFFFFFF], [0, 0x80000000, 0, 0x3FFFFFFF]], dtype=np.uint32)
    u = _uniform(r)
    assert u.min() == np.float32(2.0 ** -33) and u.max() == np.float32(1.0)
    z = _box_muller(r)
    assert np.isfinite(z).all() and np.abs(z).max() <= 6.77
    assert abs(np.abs(z).max() - np.sqrt(66 * np.log(2.0))) < 1e-9      # sqrt(-2 ln 2^-33) = 6.764


BIG_OFFSET = (1 << 36) + 4 * 12345      # counter index 2^34 + 12345: the high counter word is 4
SEEDS = [0, 1234, (1 << 32) + 77, (1 << 63) - 1]


@gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_device_randn_against_the_cpu_generator(seed):
    from mi355.ops import default_ops as ops

    worst = 0.0
    for offset in (0, 4, BIG_OFFSET):
        for n in (4096, 4099, 5, 1):
            got = ops.randn((n,), DEV, seed, offset).cpu().double().numpy()
            want = reference_randn(seed, offset, n)
            err = np.abs(got - want).max()
            worst = max(worst, err)
            # the fp32 angle 2 pi u (rounded product, rounded constant) is off by <= 2 pi (2^-24 + 2.8e-8) = 5.5e-7, times the largest
            # radius 6.77: 3.7e-6; logf, sqrtf, sinf, cosf add a few ulp of values <= 6.77 (4e-7 each).  A structural defect (rounds,
            # counter words, key schedule, lane order) gives differences of order 1.
            assert err <= 1e-5, (seed, offset, n, err)
    z = ops.randn((1 << 16,), DEV, seed, 0).cpu().double().numpy()
    assert np.abs(z - reference_randn(seed, 0, 1 << 16)).max() <= 1e-5
    print(f"randn seed {seed}: worst |device - fp64 Box-Muller of the numpy Philox| = {worst:.2e}")
    # measured on an MI355X: 9.5e-07, 1.14e-06, 1.12e-06, 1.04e-06 for the four seeds


@gpu
def test_device_randn_does_not_write_past_a_ragged_tail():
    """mi355_randn through the C entry point into a guarded buffer (the op wrapper allocates its own output)."""
    import ctypes as C

    from mi355 import _lib

    for n in (1, 5, 4099):
        buf = torch.full((n + 8,), -777.25, device=DEV)
        _lib.check(_lib.lib().mi355_randn(C.c_void_p(buf.data_ptr()), 1234, 8, n, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        got = buf.cpu()
        assert (got[n:] == -777.25).all()
        assert np.abs(got[:n].double().numpy() - reference_randn(1234, 8, n)).max() <= 1e-5


# ---- offset contract -------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("offset", [1, 2, 5, BIG_OFFSET + 3])
def test_a_philox_offset_that_is_not_a_multiple_of_4_is_refused(offset):
    """One Philox counter yields 4 elements: an offset inside a counter cannot be honoured, and flooring it silently would hand out a
    different part of the stream than the caller asked for."""
    from mi355._lib import MI355BackendError
    from mi355.ops import default_ops as ops

    x, e = randn(1, 64).to(DEV), randn(2, 64).to(DEV)
    before = x.clone()
    with pytest.raises(MI355BackendError, match="multiple of 4"):
        ops.randn((64,), DEV, 7, offset)
    with pytest.raises(MI355BackendError, match="multiple of 4"):
        ops.ddpm_step_(x, e, None, 1.5, 1.1, 0.1, 0.9, 0.3, philox=(7, offset))
    with pytest.raises(MI355BackendError, match="multiple of 4"):
        ops.corrector_step_(x, e, None, 1.5, 1.1, 0.9, 0.04, 0.1, philox=(7, offset))
    with pytest.raises(MI355BackendError, match="multiple of 4"):
        ops.replace_mask_(x, e, None, -2.0, True, 0.8, 0.6, philox=(7, offset))
    with pytest.raises(MI355BackendError, match="multiple of 4"):
        ops.sde_euler_step_(x, e, 0.1, 0.5, philox=(7, offset))
    assert torch.equal(x, before)       # a refused call launches nothing
    ops.randn((64,), DEV, 7, offset // 4 * 4 + 4)   # the neighbouring multiple is fine


# ---- Philox branch == injected branch, kernel by kernel ------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", [4096, 4099])
@pytest.mark.parametrize("kernel", ["ddpm_step", "corrector_step", "replace_mask"])
def test_philox_branch_equals_injected_branch(kernel, n):
    from mi355.ops import default_ops as ops

    seed = (1 << 40) + 99
    off = 3 * ((n + 3) // 4 * 4)
    x, e = randn(3, n).to(DEV), randn(4, n).to(DEV)
    cond = rand_uniform(5, -1.0, 1.0, n)
    cond[::3] = -2.0
    cond = cond.to(DEV)
    z = ops.randn((n,), DEV, seed, off)

    def run(zz, ph):
        y = x.clone()
        if kernel == "ddpm_step":
            return ops.ddpm_step_(y, e, zz, 1.25, 0.75, 0.12, 0.85, 0.3, philox=ph)
        if kernel == "corrector_step":
            return ops.corrector_step_(y, e, zz, 1.25, 0.75, 1.33, 0.04, 0.1, philox=ph)
        return ops.replace_mask_(y, cond, zz, -2.0, True, 0.8, 0.6, philox=ph)

    injected, device, silent = run(z, None), run(None, (seed, off)), run(None, None)
    assert torch.equal(device, injected)
    assert not torch.equal(device, silent)                          # the noise term is there at all
    assert not torch.equal(device, run(None, (seed, off + 4)))      # ... and comes from this offset
    assert not torch.equal(device, run(None, (seed + 1, off)))      # ... of this seed


# ---- the whole sampler: call k draws at offset k * n_al ---------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("mode", ["prior", "amortized_corrector", "replacement_noisy"])
def test_ddpm_sample_device_noise_is_the_documented_stream(mode):
    """mi355_ddpm_sample numbers its torch.randn_like calls in the reference's order (per step i = Ns-1 .. 0: the replacement q_sample,
    the predictor's z iff i > 0, one per corrector step) and, with noise == NULL, takes call k from (seed, offset k * n_al)."""
    from image_diffusion.sde_diffusion import DDPM
    from mi355 import _lib
    from mi355.ops import default_ops as ops
    from tests.test_gpu_unet import _tiny

    Ns, S, B = 25, (1 << 33) + 5, 2
    ddpm = DDPM(Ns)
    tables = ddpm.host_tables()
    x0 = randn(21, B, 3, 16, 16)
    cond = rand_uniform(22, -1.0, 1.0, B, 3, 16, 16)
    cond[:, :, 4:12, 4:12] = -2.0
    if mode == "prior":
        _, net, _ = _tiny(3, 3, 1001, "fp32")
        kw, n_draws = dict(mode=_lib.DDPM_PRIOR), Ns - 1
    elif mode == "amortized_corrector":
        _, net, _ = _tiny(6, 3, 1002, "fp32")
        kw, n_draws = dict(mode=_lib.DDPM_AMORTIZED, cond=cond.to(DEV), n_corrector=1, delta=0.1), (Ns - 1) + Ns
    else:
        _, net, _ = _tiny(3, 3, 1003, "fp32")
        kw = dict(mode=_lib.DDPM_REPLACEMENT, cond=cond.to(DEV), noise_condition=True, start_fraction=1.0, pad_value=-2.0)
        n_draws = Ns + (Ns - 1)
    eng = net.engine(torch.device(DEV))
    n = x0.numel()
    n_al = (n + 3) // 4 * 4
    device = eng.ddpm_sample(x0.to(DEV).clone(), tables, noise=None, seed=S, **kw).cpu()
    draws = torch.stack([ops.randn(tuple(x0.shape), DEV, S, k * n_al) for k in range(n_draws)])
    injected = eng.ddpm_sample(x0.to(DEV).clone(), tables, noise=draws, seed=0, **kw).cpu()
    assert torch.isfinite(device).all() and float(device.abs().max()) <= 1.0
    assert torch.equal(device, injected)
    # one draw fewer is refused (the count is the documented one), another seed gives another sample
    from mi355._lib import MI355BackendError
    with pytest.raises(MI355BackendError, match="exhausted"):
        eng.ddpm_sample(x0.to(DEV).clone(), tables, noise=draws[:-1].contiguous(), seed=0, **kw)
    other = eng.ddpm_sample(x0.to(DEV).clone(), tables, noise=None, seed=S + 1, **kw).cpu()
    assert not torch.equal(other, device)
