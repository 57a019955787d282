"""GPU op tests of the step's noise, latent, loss and optimizer kernels (lunaris_orion_amd/csrc/lo_train.hip) through the C ABI,
each against a plain float64 restatement of the same operation on the same inputs.

Every device buffer comes from tests/guarded.py (exactly the ABI's element count, 1 MiB of guard band on each side, outputs
pre-filled with a sentinel), so "every element written" and "nothing beyond written" are part of each test; the *_aligned16 tests
run one case per op with every pointer at (256 B multiple) + 16 B, the alignment include/lunaris_hip.h promises.

Bounds and what was measured on MI355X (worst over all cases of the test named; the tests print every figure before asserting):

  noise, elementwise      |lo_reparam_noise - float64 restatement| (oracle/noise_ref.py; __logf / __cosf against log / cos):
                          measured 2.046e-6 (NOISE_MEASURED), bound NOISE_ABS_BOUND = 4 x measured = 8.2e-6; the bound may not
                          exceed 1e-3, above which the moment limits of oracle/noise_ref.py would no longer resolve the error.
  noise, statistics       the conditions of oracle/noise_ref.py (assert_standard_normal / assert_uncorrelated), unchanged, on the
                          device's vectors.
  head reduce             mu, logvar: (nsplit + 1) 2^-23 sum|terms| per element (nsplit + 1 fp32 terms added in order: nsplit
                          roundings of at most 2^-24 of the running sum each); z, dml: one fp16 ulp of fp16(float64 value); KL
                          partials: 256 2^-23 sum|terms of the block|.
  loss finalise           4 x 2^-24 relative on the four losses and the two coefficients (double sums on the device; at most four
                          fp32 roundings behind them with the weights used here, which avoid cancellation in vae_loss).
  column sum              M 2^-23 sum|column| (M fp32 additions in a fixed order and the product with `scale`).
  clip + AdamW            norm: 1e-4 relative (the project's bound, tests/test_ops_gpu.py); measured 8.4e-8.  Clip
                          coefficient against max_norm / (norm64 + 1e-6) capped at 1: the same 1e-4; measured 8.8e-8; exactly 1
                          when unclipped.  After each of k steps, against float64 AdamW on the fp32-rounded hyper-parameters and the
                          device's own clip coefficient: |p - p64| <= k 2^-22 max(1, |p64|), |m - m64| <= k 2^-22 max|m64|,
                          |v - v64| <= k 2^-22 max|v64| (per step: p two roundings of 2^-24 |p| and the rounding of the decay
                          factor, m three roundings, v at most five -- each below 4 x 2^-24 = 2^-22 of the value).  Worst measured
                          error / bound: p 0.55, m 0.88, v 0.64 (m: the one-element case, where the second step's gradient has the
                          opposite sign and m is the difference of two close terms; 0.36 everywhere else).
"""
import math

import numpy as np
import pytest
import torch

from oracle import noise_ref as N
from tests.guarded import check_guards, gin, guarded, written
from tests.hip_helpers import L as _L, sync

pytestmark = pytest.mark.gpu

NOISE_MEASURED = 2.046e-6                  # worst |device - float64| on MI355X over all seeds and spans below
NOISE_ABS_BOUND = 4 * NOISE_MEASURED
U24, U23, U22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22


def _call(name, *args):
    lib = _L()
    lib.check(getattr(lib.lib, name)(*args), name)


def _st():
    return _L().stream_ptr()


def _p(t):
    return None if t is None else t.data_ptr()


def _np(t):
    return t.detach().cpu().double().numpy()


def _ulp16(y):
    """Spacing of fp16 at the (fp16-representable, float64) values y; 2^-24 in the subnormal range."""
    e = np.floor(np.log2(np.maximum(np.abs(y), 2.0 ** -14)))
    return 2.0 ** (e - 10)


def _assert_fp16_within_one_ulp(got_f16, ref64, what):
    got = _np(got_f16).reshape(-1)
    assert np.isfinite(got).all(), f"{what}: not finite"
    ref16 = ref64.reshape(-1).astype(np.float16).astype(np.float64)
    d = np.abs(got - ref16) / _ulp16(ref16)
    print(f"MEASURED {what}: worst |device - fp16(float64)| = {d.max():.3g} fp16 ulp, {int((d > 0).sum())} of {d.size} differ")
    assert d.max() <= 1.0, (what, float(d.max()), int(d.argmax()))


# =================================================================================================
# A. the N(0,1) generator
# =================================================================================================
_ref_cache, _dev_cache = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_the_noise_vectors_afterwards():
    yield
    _ref_cache.clear()
    _dev_cache.clear()


def _ref_vector(seed):
    """The restatement's float64 samples 0 .. 2^20 + 20000 of one call seed (computed once per module run)."""
    if seed not in _ref_cache:
        _ref_cache[seed] = N.randn(seed, 0, N.STAT_N + 20000)
    return _ref_cache[seed]


def _noise(seed, first, n, skew=0):
    out = guarded(n, torch.float32, "out", skew)
    _call("lo_reparam_noise", seed, first, n, out.data_ptr(), _st())
    sync()
    written(out)
    check_guards(out)
    return out


def _dev_vector(seed):
    if seed not in _dev_cache:
        _dev_cache[seed] = _noise(seed, 0, N.STAT_N).cpu().numpy()
    return _dev_cache[seed]


NOISE_SPANS = [(0, 1), (0, 63), (0, 64), (0, 65), (0, N.STAT_N), (12345, 4099)]


@pytest.mark.parametrize("torch_seed", N.STAT_TORCH_SEEDS)
def test_reparam_noise_matches_the_restatement(torch_seed):
    """Element by element against oracle/noise_ref.py, for the first four call seeds of both ranks' streams of this torch seed.
    Measured on MI355X: worst |device - float64| = 2.046e-6 over all seeds and spans; the bound is four times that, 8.2e-6."""
    worst = 0.0
    for rank in N.STAT_RANKS:
        for seed in N.call_seeds(torch_seed, rank, N.STAT_CALLS):
            ref = _ref_vector(seed)
            for first, n in NOISE_SPANS:
                got = _dev_vector(seed) if (first, n) == (0, N.STAT_N) else _noise(seed, first, n).cpu().numpy()
                assert got.shape == (n,) and got.dtype == np.float32
                err = float(np.abs(got.astype(np.float64) - ref[first:first + n]).max())
                worst = max(worst, err)
                assert err <= NOISE_ABS_BOUND, (hex(seed), first, n, err)
    print(f"MEASURED noise torch_seed={torch_seed}: worst |device - float64| = {worst:.4g} (bound {NOISE_ABS_BOUND:.4g})")
    assert NOISE_ABS_BOUND <= 1e-3


def test_reparam_noise_at_the_generators_edge_points():
    """u1 == 1.0 (radius exactly 0) and k1 == 0 (u1 = 2^-25, the largest radius): finite, within the elementwise bound."""
    for idx in (N.EDGE_INDEX_U1_ONE, N.EDGE_INDEX_K1_ZERO):
        got = _noise(N.EDGE_SEED, idx - 1, 3).cpu().numpy().astype(np.float64)          # the point and its two neighbours
        ref = N.randn(N.EDGE_SEED, idx - 1, 3)
        print(f"MEASURED noise edge index {idx}: device {got[1]!r} float64 {ref[1]!r}")
        assert np.isfinite(got).all() and np.abs(got - ref).max() <= NOISE_ABS_BOUND, (idx, got, ref)
        one = _noise(N.EDGE_SEED, idx, 1).cpu().numpy()
        assert one[0] == np.float32(got[1])
    assert _noise(N.EDGE_SEED, N.EDGE_INDEX_U1_ONE, 1).cpu().numpy()[0] == 0.0


def test_reparam_noise_aligned16():
    seed = N.call_seed(42, 1, 3)
    got = _noise(seed, 12345, 4099, skew=16).cpu().numpy()
    assert np.abs(got.astype(np.float64) - _ref_vector(seed)[12345:12345 + 4099]).max() <= NOISE_ABS_BOUND


@pytest.mark.parametrize("torch_seed", N.STAT_TORCH_SEEDS)
@pytest.mark.parametrize("rank", N.STAT_RANKS)
def test_reparam_noise_is_standard_normal_on_the_device(torch_seed, rank):
    """The conditions tests/test_noise_ref.py puts on the restatement, on the device's own vectors of 2^20 samples."""
    vec = [_dev_vector(s) for s in N.call_seeds(torch_seed, rank, N.STAT_CALLS)]
    for k, x in enumerate(vec, start=1):
        st = N.statistics(x)
        print(f"MEASURED noise statistics torch_seed={torch_seed} rank={rank} forward={k}: " + " ".join(f"{a}={b:.3e}" for a, b in st.items()))
        N.assert_standard_normal(st, (torch_seed, rank, k))
        if k > 1:
            N.assert_uncorrelated(x, vec[k - 2], (torch_seed, rank, "forward", k, "with the one before"))
    if rank == 1:
        for k, s0 in enumerate(N.call_seeds(torch_seed, 0, N.STAT_CALLS), start=1):
            N.assert_uncorrelated(_dev_vector(s0), vec[k - 1], (torch_seed, "rank 0 with rank 1 at forward", k))


def _vae(latent):
    from lunaris_orion_amd.vae import LunarisCoreVAE
    from oracle import vae_ref as R
    m = LunarisCoreVAE(latent_dim=latent)
    m.load_state_dict(R.closed_form_params(latent))
    return m.to("cuda")


@pytest.mark.parametrize("B", [2, 5])
def test_forward_draws_the_noise_of_its_stream(B):
    """What lo_vae_forward applies with eps = NULL is lo_reparam_noise of the stream's call seed: forward k of a model (k = 1, 2, 3)
    equals, bit for bit in the reconstruction, a second model's forward handed that noise explicitly -- with the seeds taken from
    the restatement (torch seed, rank 0, forward k), not from the model, so a stream that does not advance fails too.  A model whose
    `noise_calls` was restored to 2 (hostside.load_checkpoint) reproduces the third forward."""
    from oracle import vae_ref as R
    latent, ts = 64, 1234
    x = R.normalise_sprites(R.closed_form_sprites(B)).cuda()
    torch.manual_seed(ts)
    assert torch.initial_seed() == ts
    seeds = N.call_seeds(ts, 0, 3)
    free, given = _vae(latent), _vae(latent)
    recon_free, noise = [], []
    with torch.no_grad():
        for k in range(3):
            r, _mu, _lv = free(x)
            sync()
            assert free._seed == seeds[k] and free.noise_calls == k + 1
            recon_free.append(r.cpu())
            e = _noise(seeds[k], 0, B * latent)
            noise.append(e.cpu())
            r2, _mu2, _lv2 = given(x, e.view(B, latent).clone())
            sync()
            assert torch.equal(recon_free[k], r2.cpu()), f"forward {k + 1}: eps = NULL is not lo_reparam_noise of call seed {k + 1}"
        assert not torch.equal(noise[0], noise[1]) and not torch.equal(noise[1], noise[2])
        assert not torch.equal(recon_free[0], recon_free[1]) and not torch.equal(recon_free[1], recon_free[2])
        resumed = _vae(latent)
        resumed._seed, resumed.noise_calls = None, 2                    # as hostside restores a checkpoint's stream position
        r3, _mu3, _lv3 = resumed(x)
        sync()
        assert resumed._seed == seeds[2] and resumed.noise_calls == 3
        assert torch.equal(r3.cpu(), recon_free[2])


# =================================================================================================
# B. latent head, its backward, loss finalisation, column sums
# =================================================================================================
LATENT_SHAPES = [(1, 64, 1), (3, 64, 7), (5, 64, 9), (2, 256, 32), (7, 128, 17)]


def _head_reduce(B, Ld, nsplit, skew=0, user=False):
    g = torch.Generator().manual_seed(1000 * B + Ld + nsplit)
    slab = torch.randn(nsplit, B, 2 * Ld, generator=g) / math.sqrt(nsplit)
    bias = torch.randn(2 * Ld, generator=g) * 0.1
    eps = torch.randn(B * Ld, generator=g)
    n, nb = B * Ld, (B * Ld + 255) // 256
    slab_d, bias_d, eps_d = gin(slab, skew), gin(bias, skew), gin(eps, skew)
    mu, lv, eo = (guarded(n, torch.float32, "out", skew) for _ in range(3))
    z = guarded(n, torch.float16, "out", skew)
    klp = guarded(nb, torch.float32, "out", skew)
    mu_u = guarded(n, torch.float32, "out", skew) if user else None
    lv_u = guarded(n, torch.float32, "out", skew) if user else None
    _call("lo_latent_forward_op", slab_d.data_ptr(), bias_d.data_ptr(), eps_d.data_ptr(), 0, mu.data_ptr(), lv.data_ptr(), z.data_ptr(),
          eo.data_ptr(), klp.data_ptr(), B, Ld, nsplit, _p(mu_u), _p(lv_u), _st())
    sync()
    written(mu, lv, eo, z, klp, mu_u, lv_u)
    s64, b64 = _np(slab), _np(bias)
    tot = b64[None, :] + s64.sum(0)                                   # [B][2L], float64 sums of the fp32 terms
    mag = np.abs(b64)[None, :] + np.abs(s64).sum(0)
    m64, l64 = tot[:, :Ld].reshape(-1), tot[:, Ld:].reshape(-1)
    bm, bl = (nsplit + 1) * U23 * mag[:, :Ld].reshape(-1), (nsplit + 1) * U23 * mag[:, Ld:].reshape(-1)
    em, el = np.abs(_np(mu) - m64), np.abs(_np(lv) - l64)
    print(f"MEASURED head reduce ({B},{Ld},{nsplit}): worst error / bound mu {np.max(em / bm):.3g} logvar {np.max(el / bl):.3g}")
    assert (em <= bm).all() and (el <= bl).all()
    assert torch.equal(eo.cpu(), eps), "eps_out is not the noise that was passed in"
    if user:
        assert torch.equal(mu_u, mu) and torch.equal(lv_u, lv)
    _assert_fp16_within_one_ulp(z, m64 + _np(eps) * np.exp(0.5 * l64), f"head reduce ({B},{Ld},{nsplit}) z")
    t = np.zeros(nb * 256)
    t[:n] = 1.0 + l64 - m64 * m64 - np.exp(l64)
    t = t.reshape(nb, 256)
    kl64, bk = t.sum(1), 256 * U23 * np.abs(t).sum(1)
    ek = np.abs(_np(klp) - kl64)
    print(f"MEASURED head reduce ({B},{Ld},{nsplit}): KL partials worst error / bound {np.max(ek / bk):.3g}")
    assert klp.numel() == nb and (ek <= bk).all(), (ek, bk)
    check_guards(slab_d, bias_d, eps_d, mu, lv, eo, z, klp, mu_u, lv_u)


@pytest.mark.parametrize("B,Ld,nsplit", LATENT_SHAPES)
def test_head_reduce(B, Ld, nsplit):
    _head_reduce(B, Ld, nsplit)


def test_head_reduce_aligned16():
    _head_reduce(5, 64, 9, skew=16, user=True)


def test_head_reduce_without_eps_draws_lo_reparam_noise():
    """eps_in = NULL: eps_out is lo_reparam_noise(seed, 0, B L) bit for bit, and z is built from it."""
    B, Ld, nsplit, seed = 5, 64, 3, N.call_seed(1, 0, 2)
    g = torch.Generator().manual_seed(7)
    slab, bias = torch.randn(nsplit, B, 2 * Ld, generator=g) * 0.5, torch.randn(2 * Ld, generator=g) * 0.1
    n, nb = B * Ld, (B * Ld + 255) // 256
    slab_d, bias_d = gin(slab), gin(bias)
    mu, lv, eo = (guarded(n, torch.float32, "out") for _ in range(3))
    z, klp = guarded(n, torch.float16, "out"), guarded(nb, torch.float32, "out")
    _call("lo_latent_forward_op", slab_d.data_ptr(), bias_d.data_ptr(), None, seed, mu.data_ptr(), lv.data_ptr(), z.data_ptr(), eo.data_ptr(),
          klp.data_ptr(), B, Ld, nsplit, None, None, _st())
    sync()
    written(mu, lv, eo, z, klp)
    assert torch.equal(eo.cpu(), _noise(seed, 0, n).cpu())
    _assert_fp16_within_one_ulp(z, _np(mu) + _np(eo) * np.exp(0.5 * _np(lv)), "head reduce, device noise, z")
    check_guards(slab_d, bias_d, mu, lv, eo, z, klp)


def _latent_backward(B, Ld, path, skew=0):
    g = torch.Generator().manual_seed(77 * B + Ld)
    n = B * Ld
    dz = (torch.randn(n, generator=g) * 1.5).to(torch.float16)
    mu, eps = torch.randn(n, generator=g), torch.randn(n, generator=g)
    lv = torch.rand(n, generator=g) * 9.0 - 6.0                       # [-6, 3]
    coefs = torch.tensor([123.0, 0.37], dtype=torch.float32)
    gmu, glv, gscale = torch.randn(n, generator=g), torch.randn(n, generator=g), 0.75
    use_c, use_m, use_l = {"fused": (True, False, False), "explicit": (False, True, True), "mixed": (True, True, False)}[path]
    dz_d, mu_d, lv_d, eps_d = gin(dz, skew), gin(mu, skew), gin(lv, skew), gin(eps, skew)
    c_d = gin(coefs, skew) if use_c else None
    gm_d = gin(gmu, skew) if use_m else None
    gl_d = gin(glv, skew) if use_l else None
    dml = guarded((B, 2 * Ld), torch.float16, "out", skew)
    _call("lo_latent_backward_op", dz_d.data_ptr(), mu_d.data_ptr(), lv_d.data_ptr(), eps_d.data_ptr(), _p(c_d), _p(gm_d), _p(gl_d), gscale,
          dml.data_ptr(), B, Ld, _st())
    sync()
    written(dml)
    ckl = float(coefs[1]) if use_c else 0.0
    d, m64, l64, e64 = _np(dz), _np(mu), _np(lv), _np(eps)
    dm = ckl * m64 + d + (gscale * _np(gmu) if use_m else 0.0)
    dl = ckl * 0.5 * (np.exp(l64) - 1.0) + d * e64 * 0.5 * np.exp(0.5 * l64) + (gscale * _np(glv) if use_l else 0.0)
    ref = np.concatenate([dm.reshape(B, Ld), dl.reshape(B, Ld)], axis=1)
    _assert_fp16_within_one_ulp(dml, ref, f"latent backward ({B},{Ld}) {path}")
    check_guards(dz_d, mu_d, lv_d, eps_d, c_d, gm_d, gl_d, dml)


@pytest.mark.parametrize("path", ["fused", "explicit", "mixed"])
@pytest.mark.parametrize("B,Ld,nsplit", LATENT_SHAPES)
def test_latent_backward(B, Ld, nsplit, path):
    _latent_backward(B, Ld, path)


def test_latent_backward_aligned16():
    _latent_backward(7, 128, "mixed", skew=16)


def _loss_finalize(n_mse, skew=0):
    g = torch.Generator().manual_seed(n_mse)
    f32 = lambda v: float(np.float32(v))
    rw, kw, ls = f32(1.0), f32(0.05), f32(65536.0)
    for n_kl in (1, 3, 256):
        mse = torch.rand(n_mse, generator=g) * 40.0 + 1.0
        kl = torch.randn(n_kl, generator=g) * 30.0 - 50.0
        mse_d, kl_d = gin(mse, skew), gin(kl, skew)
        n_rec, n_lat = float(n_mse // 64 * 49152), float(n_kl * 256)
        for adv_host, adv_dev in ((0.125, None), (7.0, 0.3)):         # the device scalar overrides the host value
            for accum in (1.0, 4.0):
                adv_d = gin(torch.tensor([adv_dev], dtype=torch.float32), 0) if adv_dev is not None else None
                losses, coefs = guarded(4, torch.float32, "out", skew), guarded(2, torch.float32, "out", skew)
                _call("lo_loss_finalize_op", mse_d.data_ptr(), n_mse, kl_d.data_ptr(), n_kl, rw, kw, adv_host, _p(adv_d), accum, ls,
                      losses.data_ptr(), coefs.data_ptr(), n_rec, n_lat, _st())
                sync()
                written(losses, coefs)
                adv = f32(adv_dev if adv_dev is not None else adv_host)
                recon = _np(mse).sum() / n_rec
                kll = -0.5 * _np(kl).sum() / n_lat
                pg = -adv * recon
                ref = np.array([recon, kll, (rw * recon + kw * kll + pg) / accum, pg, ls * (rw - adv) / accum * 2.0 / n_rec, ls * kw / accum / n_lat])
                got = np.concatenate([_np(losses), _np(coefs)])
                rel = np.abs(got - ref) / np.abs(ref)
                print(f"MEASURED loss finalise n_mse={n_mse} n_kl={n_kl} adv={adv} accum={accum}: worst relative error {rel.max() / U24:.3g} x 2^-24")
                assert (rel <= 4 * U24).all(), (n_mse, n_kl, adv, accum, got, ref)
                check_guards(mse_d, kl_d, adv_d, losses, coefs)


@pytest.mark.parametrize("n_mse", [64, 2048, 2112, 8192])
def test_loss_finalize(n_mse):
    _loss_finalize(n_mse)


def test_loss_finalize_aligned16():
    _loss_finalize(2112, skew=16)


def _colsum(M, Nc, skew=0):
    g = torch.Generator().manual_seed(M * 100003 + Nc)
    x = torch.randn(M, Nc, generator=g).to(torch.float16)
    scale = float(np.float32(0.37))
    x_d = gin(x, skew)
    out = guarded(Nc, torch.float32, "out", skew)
    _call("lo_colsum_f16_op", x_d.data_ptr(), out.data_ptr(), M, Nc, scale, _st())
    sync()
    written(out)
    x64 = _np(x)
    ref, bound = scale * x64.sum(0), M * U23 * scale * np.abs(x64).sum(0)
    err = np.abs(_np(out) - ref)
    print(f"MEASURED column sum ({M},{Nc}): worst error / bound {np.max(err / bound):.3g}")
    assert (err <= bound).all(), (M, Nc, int(np.argmax(err / bound)))
    check_guards(x_d, out)                                            # columns past N: nothing written


@pytest.mark.parametrize("M,Nc", [(1, 128), (7, 128), (9, 640), (33, 1032), (40, 32768), (128 * 64, 640)])
def test_colsum_f16(M, Nc):
    _colsum(M, Nc)


def test_colsum_f16_aligned16():
    _colsum(9, 640, skew=16)


@pytest.mark.parametrize("Nc", [4, 100, 1028])
def test_colsum_f16_refuses_a_width_that_is_no_multiple_of_8(Nc):
    lib = _L()
    x_d, out = gin(torch.zeros(3, Nc, dtype=torch.float16)), guarded(Nc, torch.float32, "out")
    assert lib.lib.lo_colsum_f16_op(x_d.data_ptr(), out.data_ptr(), 3, Nc, 1.0, _st()) == -1
    assert b"multiple of 8" in lib.lib.lo_last_error()
    sync()
    assert bool(torch.isnan(out).all())                               # nothing was launched
    check_guards(x_d, out)


# =================================================================================================
# C. clip + AdamW
# =================================================================================================
HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
MAX_NORM = 1.0


def _adamw64(p, g, m, v, coef, step, wd):
    """One float64 AdamW step (torch.optim.AdamW's arithmetic) on the fp32-rounded hyper-parameters; returns new (p, m, v)."""
    lr, b1, b2, eps, wd = (float(np.float32(t)) for t in (HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], wd))
    gg = g * coef
    m = m + (gg - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * gg * gg
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    p = p * (1.0 - lr * wd) - (lr / bc1) * m / (np.sqrt(v) / math.sqrt(bc2) + eps)
    return p, m, v


def _grad_with_norm(n, norm, gen):
    g = torch.randn(n, generator=gen, dtype=torch.float64)
    return (g * (norm / g.norm())).float()


def _check_state(pd, md, vd, p64, m64, v64, k, what):
    ep = np.abs(_np(pd) - p64) / (k * U22 * np.maximum(1.0, np.abs(p64)))
    em = np.abs(_np(md) - m64) / (k * U22 * np.abs(m64).max())
    ev = np.abs(_np(vd) - v64) / (k * U22 * np.abs(v64).max())
    print(f"MEASURED adamw {what} after step {k}: worst error / bound p {ep.max():.3g} m {em.max():.3g} v {ev.max():.3g}")
    assert ep.max() <= 1.0 and em.max() <= 1.0 and ev.max() <= 1.0, (what, k, ep.max(), em.max(), ev.max())


ADAMW_LENGTHS = [1, 2, 3, 4, 5, 1023, 1024, 262144, 1048576, 1048580, 786441]
ADAMW_VARIANTS = [("unclipped", 0.01, 1), ("clipped", 0.0, 1), ("clipped", 0.01, 100000), ("unclipped", 0.0, 100000)]


def _clip_adamw(n, clip, wd, step0, skew=0):
    gen = torch.Generator().manual_seed(n + step0)
    p = torch.randn(n, generator=gen)
    pd, md, vd = gin(p, skew), gin(torch.zeros(n), skew), gin(torch.zeros(n), skew)
    scratch = gin(torch.zeros(1028), skew)
    p64, m64, v64 = _np(p), np.zeros(n), np.zeros(n)
    target = (0.5 if clip == "unclipped" else 10.0) * MAX_NORM
    for k in range(1, 4):
        grad = _grad_with_norm(n, target * (1.0 + 0.1 * (k - 1)), gen)
        gd = gin(grad, skew)
        _call("lo_clip_adamw_step", pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, MAX_NORM, HYPER["lr"], HYPER["beta1"],
              HYPER["beta2"], HYPER["eps"], wd, step0 + k - 1, scratch.data_ptr(), _st())
        sync()
        s = scratch[1024:1028].cpu().double().numpy()
        norm64 = float(np.sqrt((_np(grad) ** 2).sum()))
        coef64 = min(1.0, MAX_NORM / (norm64 + 1e-6))
        print(f"MEASURED adamw n={n} {clip} step {k}: norm relative error {abs(s[0] - norm64) / norm64:.3g}, "
              f"coefficient relative error {abs(s[1] - coef64) / coef64:.3g}")
        assert abs(s[0] - norm64) <= 1e-4 * norm64
        assert s[2] == 1.0 and s[3] == 0.0
        if clip == "unclipped":
            assert s[1] == 1.0
        else:
            assert abs(s[1] - coef64) <= 1e-4 * coef64 and s[1] < 0.2
        p64, m64, v64 = _adamw64(p64, _np(grad), m64, v64, s[1], step0 + k - 1, wd)
        _check_state(pd, md, vd, p64, m64, v64, k, f"n={n} {clip} wd={wd} first step {step0}")
        check_guards(pd, gd, md, vd, scratch)


@pytest.mark.parametrize("clip,wd,step0", ADAMW_VARIANTS)
@pytest.mark.parametrize("n", ADAMW_LENGTHS)
def test_clip_adamw(n, clip, wd, step0):
    _clip_adamw(n, clip, wd, step0)


def test_clip_adamw_aligned16():
    _clip_adamw(1023, "clipped", 0.01, 1, skew=16)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32).clone()


def _adamw_range(pd, gd, md, vd, n, norm_ptr, wd, step, cast):
    _call("lo_adamw_range", pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, norm_ptr, HYPER["lr"], HYPER["beta1"], HYPER["beta2"],
          HYPER["eps"], wd, step, _p(cast), _st())
    sync()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_a_non_finite_gradient_skips_the_update(bad):
    """One inf / NaN among the gradients: p, m, v and lo_adamw_range's fp16 copy stay as they were, bit for bit; scratch[1026] == 0;
    scratch[1027] counts 1, 2; a finite step afterwards updates and leaves the count."""
    n, wd = 1027, 0.01                                                # vector body and a three-element tail
    gen = torch.Generator().manual_seed(5)
    pd, md, vd = gin(torch.randn(n, generator=gen)), gin(torch.zeros(n)), gin(torch.zeros(n))
    scratch = gin(torch.zeros(1028))
    step = lambda gd, k: _call("lo_clip_adamw_step", pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, MAX_NORM, HYPER["lr"],
                               HYPER["beta1"], HYPER["beta2"], HYPER["eps"], wd, k, scratch.data_ptr(), _st())
    g1 = gin(_grad_with_norm(n, 3.0, gen))
    step(g1, 1)                                                       # a finite step first: m and v are no longer zero
    sync()
    before = [_bits(t) for t in (pd, md, vd)]
    assert scratch[1026].item() == 1.0 and scratch[1027].item() == 0.0
    for count, where in ((1, 500), (2, n - 1)):                       # in the vector body, in the tail
        gb = _grad_with_norm(n, 3.0, gen)
        gb[where] = bad
        gbd = gin(gb)
        step(gbd, 2)
        sync()
        assert scratch[1026].item() == 0.0 and scratch[1027].item() == float(count) and scratch[1025].item() == 0.0
        cast = guarded(n, torch.float16, "out")
        _adamw_range(pd, gbd, md, vd, n, scratch.data_ptr() + 4 * 1024, wd, 2, cast)
        assert bool((_bits(cast) == -1).all()), "the fp16 copy of a skipped update was written"
        for t, b, name in zip((pd, md, vd), before, "pmv"):
            assert torch.equal(_bits(t), b), f"{name} changed in a skipped update"
        check_guards(pd, gbd, md, vd, scratch, cast)
    g2 = gin(_grad_with_norm(n, 3.0, gen))
    step(g2, 2)
    sync()
    assert scratch[1026].item() == 1.0 and scratch[1027].item() == 2.0
    for t, b in zip((pd, md, vd), before):
        assert not torch.equal(_bits(t), b)
    check_guards(pd, g2, md, vd, scratch)


@pytest.mark.parametrize("n", [3, 5, 1027, 4096])
def test_adamw_range_cast_and_norm_forms(n):
    """lo_adamw_range: cast == fp16(p) after the update, bit for bit; norm == NULL is coefficient 1 (the bits of norm = {., 1, 1}, and
    float64 AdamW within the per-step bounds); norm[2] == 0 leaves p, m, v and a sentinel-filled cast alone."""
    gen = torch.Generator().manual_seed(n)
    p, m, v = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.01, torch.rand(n, generator=gen) * 1e-3
    grad = torch.randn(n, generator=gen) * 0.05
    wd, step = 0.01, 7
    out = {}
    for form, norm in (("null", None), ("one", [9.0, 1.0, 1.0]), ("half", [9.0, 0.5, 1.0]), ("skip", [9.0, 0.5, 0.0])):
        pd, md, vd, gd = gin(p), gin(m), gin(v), gin(grad)
        nd = gin(torch.tensor(norm, dtype=torch.float32)) if norm is not None else None
        cast = guarded(n, torch.float16, "out")
        _adamw_range(pd, gd, md, vd, n, _p(nd), wd, step, cast)
        out[form] = [_bits(t) for t in (pd, md, vd, cast)]
        check_guards(pd, md, vd, gd, nd, cast)
        if form == "skip":
            assert bool((out[form][3] == -1).all())
            for got, t in zip(out[form][:3], (p, m, v)):
                assert torch.equal(got, _bits(t))
            continue
        written(cast)
        assert torch.equal(_bits(cast), _bits(pd.cpu().to(torch.float16))), "cast is not fp16(p)"
        p64, m64, v64 = _adamw64(_np(p), _np(grad), _np(m), _np(v), 0.5 if form == "half" else 1.0, step, wd)
        _check_state(pd, md, vd, p64, m64, v64, 1, f"lo_adamw_range n={n} norm {form}")
    for a, b in zip(out["null"], out["one"]):
        assert torch.equal(a, b)
    assert not torch.equal(out["null"][0], out["half"][0])


def _dyadic_grad(n, gen):
    """Gradients on the grid k / 64, |k| <= 8: every square is a multiple of 2^-12 and every partial sum of 2^20 of them is exact in
    fp32, so the sum of squares does not depend on how it is split among workgroups or launches."""
    return torch.randint(-8, 9, (n,), generator=gen).float() / 64.0


@pytest.mark.parametrize("begin_of", [lambda n: 0, lambda n: 64, lambda n: n - 4], ids=["0", "64", "n-4"])
def test_presummed_step_equals_the_one_call_step(begin_of):
    """lo_gradnorm_early_range over [begin, n) + lo_clip_adamw_step_presummed = lo_clip_adamw_step on the same data: norm,
    coefficient, p, m, v bit for bit.  The two forms split the sum of squares among workgroups differently; with gradients whose
    partial sums are exact in fp32 (see _dyadic_grad) every split gives the same total, so equality is exact by construction."""
    n, wd = 66052, 0.01
    begin = begin_of(n)
    gen = torch.Generator().manual_seed(11)
    p, grad = torch.randn(n, generator=gen), _dyadic_grad(n, gen)
    res = []
    for form in ("one", "split"):
        pd, md, vd, gd = gin(p), gin(torch.zeros(n)), gin(torch.zeros(n)), gin(grad)
        scratch = gin(torch.zeros(1028))
        hp = (MAX_NORM, HYPER["lr"], HYPER["beta1"], HYPER["beta2"], HYPER["eps"], wd, 1, scratch.data_ptr(), _st())
        if form == "one":
            _call("lo_clip_adamw_step", pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, *hp)
        else:
            _call("lo_gradnorm_early_range", gd.data_ptr(), begin, n, scratch.data_ptr(), _st())
            _call("lo_clip_adamw_step_presummed", pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, begin, *hp)
        sync()
        check_guards(pd, md, vd, gd, scratch)
        res.append([_bits(t) for t in (scratch[1024:1028], pd, md, vd)])
    norm = res[0][0].view(torch.float32)
    norm64 = float(np.sqrt((_np(grad) ** 2).sum()))
    assert abs(norm[0].item() - norm64) <= 1e-4 * norm64 and 0.0 < norm[1].item() < 0.1 and norm[2].item() == 1.0
    for a, b, name in zip(res[0], res[1], ("norm / coefficient / flags", "p", "m", "v")):
        assert torch.equal(a, b), f"{name} differ between the one-call and the presummed form (begin {begin})"
    assert not torch.equal(res[0][1], _bits(p))


def test_gradnorm_early_range_refuses_a_begin_off_the_vector_grid():
    """begin % 4 != 0 would start 16-byte loads at a 8-byte boundary: -1, a message, nothing launched."""
    lib = _L()
    gd = gin(torch.ones(4096))
    scratch = guarded(1028, torch.float32, "out")
    assert lib.lib.lo_gradnorm_early_range(gd.data_ptr(), 6, 4096, scratch.data_ptr(), _st()) == -1
    assert b"multiple of 4" in lib.lib.lo_last_error()
    sync()
    assert bool(torch.isnan(scratch).all())
    check_guards(gd, scratch)


# =================================================================================================
# D. loss-scale helpers, transpose, sprite decode
# =================================================================================================
PICK_LENGTHS = (1, 3, 5, 4096, 1_000_003)
_pick_base = {}


def _pick_tensors():
    """The five background tensors, all |x| < 1e-3 (host copies; made once)."""
    if not _pick_base:
        gen = torch.Generator().manual_seed(3)
        _pick_base["t"] = [torch.randn(n, generator=gen).clamp_(-4, 4) * 2e-4 for n in PICK_LENGTHS]
    return [t.clone() for t in _pick_base["t"]]


def _pick(tensors, null_slot=None, skew=0):
    dev = [None if j == null_slot else gin(t, skew) for j, t in enumerate(tensors)]
    scratch = guarded(260, torch.float32, "ws", skew, payload_fill=0xFF)
    args = []
    for j, d in enumerate(dev):
        args += [_p(d), tensors[j].numel()]                           # a NULL slot keeps its (ignored) length
    _call("lo_grad_scale_pick", *args, scratch.data_ptr(), _st())
    sync()
    check_guards(scratch, *dev)
    return scratch[:3].cpu(), scratch, dev


def _assert_pick(s, true_max):
    r, inv, mx = (float(t) for t in s)
    assert _bits(s[2:3]).item() == _bits(torch.tensor([true_max], dtype=torch.float32)).item(), (mx, true_max)
    mant, _e = math.frexp(r)
    assert mant == 0.5, f"r = {r} is no power of two"
    assert 2.0 <= true_max * r < 4.0 and inv * r == 1.0, (true_max, r, inv)


@pytest.mark.parametrize("slot,index", [(3, 1001), (4, 1_000_002), (1, 2), (0, 0), (4, 500_001), (2, 4)])
@pytest.mark.parametrize("value", [3.7e4, -65536.0, 2.0 ** -7, -1.9999999])
def test_grad_scale_pick_finds_the_maximum(slot, index, value):
    """The maximum in a vector body, in a tail element, in a tail-only tensor, in the last slot; of either sign; a power of two
    (max r == 2 exactly) and just below one (max r just below 4)."""
    t = _pick_tensors()
    t[slot][index] = value
    s, _scr, _dev = _pick(t)
    _assert_pick(s, abs(float(np.float32(value))))


def test_grad_scale_pick_skips_a_null_slot_and_runs_aligned16():
    t = _pick_tensors()
    t[3][17] = 12.5
    s, _scr, _dev = _pick(t, null_slot=2)
    _assert_pick(s, 12.5)
    t[2][1] = 99.0                                                    # the maximum sits in the tensor that is then withheld
    _assert_pick(_pick(t)[0], 99.0)
    _assert_pick(_pick(t, null_slot=2, skew=16)[0], 12.5)


def test_grad_scale_pick_zero_inf_and_nan():
    """All-zero -> r = 1.  An inf -> r = 1 (and scratch[2] = inf).  A NaN does not enter the fmaxf maximum: r, 1 / r and scratch[2]
    are those of the other elements (r = 1 if they are all zero), and the NaN itself goes on through lo_scale_copy_dev."""
    zeros = [torch.zeros(n) for n in PICK_LENGTHS]
    s, _scr, _dev = _pick(zeros)
    assert s.tolist() == [1.0, 1.0, 0.0]
    t = _pick_tensors()
    t[4][77] = float("-inf")
    s, _scr, _dev = _pick(t)
    assert s.tolist() == [1.0, 1.0, float("inf")]
    for slot, index in ((3, 1002), (4, 1_000_001), (0, 0)):           # vector body, tail element, a one-element tensor
        t = _pick_tensors()
        t[1][1] = -6.0
        t[slot][index] = float("nan")
        s, scr, dev = _pick(t)
        _assert_pick(s, 6.0)
        assert s[0].item() == 0.5
        dst = guarded(t[slot].numel(), torch.float32, "out")
        _call("lo_scale_copy_dev", dev[slot].data_ptr(), dst.data_ptr(), t[slot].numel(), scr.data_ptr(), _st())
        sync()
        got = dst.cpu()
        assert math.isnan(got[index].item()) and int(torch.isnan(got).sum()) == 1
        check_guards(dst, scr, dev[slot])
    only_nan = [torch.zeros(n) for n in PICK_LENGTHS]
    only_nan[0][0] = float("nan")
    assert _pick(only_nan)[0].tolist() == [1.0, 1.0, 0.0]


@pytest.mark.parametrize("n", [1, 5, 4099])
@pytest.mark.parametrize("skew", [0, 16])
def test_scale_copy_and_unscale_by_a_device_scalar(n, skew):
    """dst = src * s and x *= s with s read from device memory: the correctly rounded fp32 products, bit for bit (s a power of two as
    lo_grad_scale_pick leaves it, and s = 0.3); a set failure word turns lo_grad_unscale_dev's result into NaN, NULL or zero do not."""
    gen = torch.Generator().manual_seed(n)
    src = torch.randn(n, generator=gen) * 100.0
    for s in (2.0 ** -9, 0.3):
        s_d, src_d = gin(torch.tensor([s], dtype=torch.float32), 0), gin(src, skew)
        want = src * torch.tensor(s, dtype=torch.float32)
        dst = guarded(n, torch.float32, "out", skew)
        _call("lo_scale_copy_dev", src_d.data_ptr(), dst.data_ptr(), n, s_d.data_ptr(), _st())
        sync()
        assert torch.equal(_bits(dst), _bits(want)) and torch.equal(src_d.cpu(), src)
        check_guards(src_d, dst, s_d)
        for word in (None, 0, 1, 0x80000000):
            x = gin(src, skew)
            w_d = gin(torch.tensor([word - (1 << 32) if word >= (1 << 31) else word], dtype=torch.int32), 0) if word is not None else None
            _call("lo_grad_unscale_dev", x.data_ptr(), n, s_d.data_ptr(), _p(w_d), _st())
            sync()
            if word:
                assert bool(torch.isnan(x).all())
            else:
                assert torch.equal(_bits(x), _bits(want))
            check_guards(x, s_d, w_d)


@pytest.mark.parametrize("rows,cols", [(64, 64), (128, 64), (64, 32768)])
def test_transpose_f16_is_bit_exact(rows, cols):
    gen = torch.Generator().manual_seed(rows + cols)
    bits = torch.randint(-32768, 32768, (rows, cols), generator=gen, dtype=torch.int32).to(torch.int16)      # every fp16 pattern, NaNs included
    src = gin(bits.view(torch.float16))
    dst = guarded((cols, rows), torch.float16, "out", payload_fill=0x00)
    _call("lo_transpose_f16", src.data_ptr(), dst.data_ptr(), rows, cols, _st())
    sync()
    assert torch.equal(_bits(dst), bits.t().contiguous())
    check_guards(src, dst)


@pytest.mark.parametrize("B", [1, 5])
def test_decode_sprites_u8_every_byte_value_in_every_channel(B):
    i = torch.arange(B * 128 * 128 * 3, dtype=torch.int64).view(B, 128, 128, 3)
    pix, ch = i // 3, i % 3
    u8 = ((pix * 7 + ch * 85 + (pix // 16384) * 31) % 256).to(torch.uint8)
    for c in range(3):
        assert len(torch.unique(u8[0, :, :, c])) == 256
    src = gin(u8)
    out = guarded((B, 3, 128, 128), torch.float32, "out")
    _call("lo_decode_sprites_u8", src.data_ptr(), out.data_ptr(), B, _st())
    sync()
    written(out)
    ref = u8.float().div(127.5).sub(1.0).permute(0, 3, 1, 2)
    assert (out.cpu() - ref).abs().max().item() <= 1.2e-7            # x/127.5 - 1 in fp32: at most 1 ulp apart
    check_guards(src, out)
