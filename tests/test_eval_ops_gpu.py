"""Op tests of the three validation kernels (csrc/lo_eval.hip) through the raw C ABI, on guard-banded buffers.

Limits and where they come from
  * per-sample sum of squared error: 1e-5 relative to a float64 restatement (49 152 fp32 squares, per-thread partial sums then a
    double tree: the fp32 part is 48 terms long);
  * SSIM: 2e-5 absolute.  The same computation in fp32 on the CPU (`fp32_vs_fp64()` below: torch's conv2d, separable, on exactly
    these inputs) differs from float64 by at most 2.9e-6 over the two input sets (the flat sample: E[x^2] - mu^2 of a constant
    cancels to the same rounding in every window, which a mean does not average away; the kernel filters x - p for that reason);
    the limit leaves 7x for the kernel's different summation order and FMA contraction.  Run it with
        python -c "import tests.test_eval_ops_gpu as t; print(t.fp32_vs_fp64())"
  * KL: 1e-6 relative (the kernel sums in double; what is left is the fp32 result's rounding, 6e-8);
  * the accumulator: 1e-12 relative on the doubles (sums of at most five doubles in another order, log10 to an ulp or two).
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C1, C2 = (0.01 * 2) ** 2, (0.03 * 2) ** 2


def _sprites(n, seed):
    """16-colour sprites of 4 x 4-pixel blocks on the uint8 grid, normalised like the dataset (x / 127.5 - 1), [n,3,128,128]."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        palette = torch.randint(0, 256, (16, 3), generator=g)
        cells = torch.randint(0, 16, (32, 32), generator=g)
        img = palette[cells].repeat_interleave(4, dim=0).repeat_interleave(4, dim=1)          # [128,128,3]
        out.append(img.permute(2, 0, 1).float() / 127.5 - 1.0)
    return torch.stack(out)


def _input_sets():
    """Two batches of three (recon, target) pairs.  A: sprites reconstructed with Gaussian noise 0.01, with noise 0.1, and by
    tanh(randn) (nothing in common).  B: a completely flat target (grey level 200) under noise 0.05, an identical pair, a sprite with
    noise 0.01."""
    g = torch.Generator().manual_seed(1234)
    noise = lambda s: s * torch.randn(3, 128, 128, generator=g)
    ta = _sprites(3, 1)
    ra = torch.stack([ta[0] + noise(0.01), ta[1] + noise(0.1), torch.tanh(torch.randn(3, 128, 128, generator=g))])
    tb = _sprites(3, 2)
    tb[0] = torch.full((3, 128, 128), 200 / 127.5 - 1.0)
    rb = torch.stack([tb[0] + noise(0.05), tb[1].clone(), tb[2] + noise(0.01)])
    return {"A": (ra.float().contiguous(), ta.contiguous()), "B": (rb.float().contiguous(), tb.contiguous())}


def metrics_ref(recon, target, dtype=torch.float64):
    """(per-sample sum of squared error, per-sample mean SSIM) restated with torch ops in `dtype`: Wang et al. 2004, 11 x 11 Gaussian
    window of sigma 1.5 normalised in double, valid positions, data range 2, variances as E[x^2] - mu^2."""
    x, y = recon.to(dtype), target.to(dtype)
    t = torch.arange(11, dtype=torch.float64) - 5
    w = torch.exp(-t * t / (2 * 1.5 ** 2))
    w = (w / w.sum()).to(dtype)

    def filt(f):
        n = f.shape[0]
        f = F.conv2d(f.reshape(n * 3, 1, 128, 128), w.view(1, 1, 1, 11))
        return F.conv2d(f, w.view(1, 1, 11, 1)).reshape(n, 3, 118, 118)
    mx, my, exx, eyy, exy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    vx, vy, cxy = exx - mx * mx, eyy - my * my, exy - mx * my
    ssim = ((2 * mx * my + C1) * (2 * cxy + C2)) / ((mx * mx + my * my + C1) * (vx + vy + C2))
    return ((x - y) ** 2).sum(dim=(1, 2, 3)), ssim.mean(dim=(1, 2, 3))


def fp32_vs_fp64():
    """Largest |SSIM(fp32) - SSIM(float64)| of the CPU restatement over the two input sets: the basis of the 2e-5 limit."""
    worst = 0.0
    for recon, target in _input_sets().values():
        worst = max(worst, (metrics_ref(recon, target, torch.float32)[1].double() - metrics_ref(recon, target)[1]).abs().max().item())
    return worst


_REF = {}


def _reference(name):
    """Inputs and float64 reference of one set, computed once for the module and left unchanged."""
    if name not in _REF:
        recon, target = _input_sets()[name]
        _REF[name] = (recon, target) + metrics_ref(recon, target)
    return _REF[name]


def _image_metrics(recon, target, n_valid):
    from lunaris_orion_amd import _lib
    from tests.guarded import check_guards, gin, guarded
    r, t = gin(recon), gin(target)
    out = guarded((recon.shape[0], 2), torch.float32, "out")
    _lib.check(_lib.lib.lo_eval_image_metrics(r.data_ptr(), t.data_ptr(), recon.shape[0], n_valid, out.data_ptr(), _lib.stream_ptr()),
               "lo_eval_image_metrics")
    torch.cuda.synchronize()
    check_guards(r, t, out)
    return out.cpu()


@pytest.mark.parametrize("name", ["A", "B"])
def test_image_metrics_match_float64_and_padding_is_invisible(name):
    recon, target, sse_ref, ssim_ref = _reference(name)
    full = _image_metrics(recon, target, 3)
    assert torch.isfinite(full).all()
    sse_err = ((full[:, 0].double() - sse_ref).abs() / sse_ref.clamp_min(1e-30)).max().item()
    ssim_err = (full[:, 1].double() - ssim_ref).abs().max().item()
    print(f"set {name}: SSE rel err {sse_err:.3e}, SSIM abs err {ssim_err:.3e}; SSIM {full[:, 1].tolist()}")
    for b in range(3):
        if sse_ref[b] == 0:
            assert full[b, 0].item() == 0.0 and full[b, 1].item() == 1.0          # an identical pair: exactly (0, 1)
        else:
            assert abs(full[b, 0].item() - sse_ref[b].item()) <= 1e-5 * sse_ref[b].item()
    assert ssim_err <= 2e-5
    if name == "B":
        assert sse_ref[1] == 0                                                     # the identical pair is in this set
    # reproducible: the same inputs give the same bits
    assert torch.equal(full, _image_metrics(recon, target, 3))
    # n_valid = 2: the third sample is padding.  NaN in both of its images stays invisible, its row is written as 0, and the valid
    # rows are the bits of the run on finite data
    rn, tn = recon.clone(), target.clone()
    rn[2], tn[2] = float("nan"), float("nan")
    part = _image_metrics(rn, tn, 2)
    assert not torch.isnan(part).any()
    assert torch.equal(part[:2], full[:2]) and torch.equal(part[2], torch.zeros(2))


@pytest.mark.parametrize("L", [64, 256])
def test_latent_kl_matches_float64(L):
    from lunaris_orion_amd import _lib
    from tests.guarded import check_guards, gin, guarded
    g = torch.Generator().manual_seed(L)
    mu = 2.0 * torch.randn(3, L, generator=g)
    logvar = torch.stack([torch.linspace(-8, 8, L)[torch.randperm(L, generator=g)] for _ in range(3)])     # spans +-8 in every sample
    ref = -0.5 * (1 + logvar.double() - mu.double() ** 2 - logvar.double().exp()).mean(dim=1)

    def run(m, lv, n_valid):
        m_d, lv_d = gin(m), gin(lv)
        out = guarded(3, torch.float32, "out")
        _lib.check(_lib.lib.lo_eval_latent_kl(m_d.data_ptr(), lv_d.data_ptr(), 3, L, n_valid, out.data_ptr(), _lib.stream_ptr()), "lo_eval_latent_kl")
        torch.cuda.synchronize()
        check_guards(m_d, lv_d, out)
        return out.cpu()
    full = run(mu, logvar, 3)
    err = ((full.double() - ref).abs() / ref.abs()).max().item()
    print(f"L={L}: KL rel err {err:.3e}")
    assert err <= 1e-6
    assert torch.equal(full, run(mu, logvar, 3))
    mn, ln = mu.clone(), logvar.clone()
    mn[2], ln[2] = float("nan"), float("nan")
    part = run(mn, ln, 2)
    assert torch.equal(part[:2], full[:2]) and part[2].item() == 0.0


@pytest.mark.parametrize("with_quality", [True, False])
def test_accumulate_two_batches_matches_float64(with_quality):
    from lunaris_orion_amd import _lib
    from tests.guarded import check_guards, gin, guarded
    g = torch.Generator().manual_seed(7)
    nan = float("nan")
    img = [torch.tensor([[812.5, 0.91], [0.0, 1.0], [30211.0, 0.12]]), torch.tensor([[3.75, 0.999], [5120.25, 0.55], [nan, nan]])]
    kl = [torch.rand(3, generator=g) * 40, torch.cat([torch.rand(2, generator=g) * 40, torch.tensor([nan])])]
    q = [torch.rand(3, 4, generator=g), torch.cat([torch.rand(2, 4, generator=g), torch.full((1, 4), nan)])]
    acc = guarded(8, torch.float64, "out")
    acc.zero_()                                                       # a zeroed accumulator starts a run
    held = []
    for b, n_valid in enumerate((3, 2)):
        bufs = (gin(img[b]), gin(kl[b]), gin(q[b]) if with_quality else None)
        held.append(bufs)
        _lib.check(_lib.lib.lo_eval_accumulate(bufs[0].data_ptr(), bufs[1].data_ptr(), _lib.ptr(bufs[2]), n_valid, acc.data_ptr(),
                                               _lib.stream_ptr()), "lo_eval_accumulate")
    torch.cuda.synchronize()
    check_guards(acc, *[t for bufs in held for t in bufs])
    got = acc.cpu().tolist()
    mse = torch.cat([img[0][:, 0], img[1][:2, 0]]).double() / 49152
    psnr = 10 * torch.log10(4 / mse.clamp_min(1e-12))
    want = [5.0, mse.sum().item(), torch.cat([kl[0], kl[1][:2]]).double().sum().item(), psnr.sum().item(),
            torch.cat([img[0][:, 1], img[1][:2, 1]]).double().sum().item(),
            torch.cat([q[0], q[1][:2]]).double().mean(dim=1).sum().item() if with_quality else 0.0, psnr.min().item(), psnr.max().item()]
    assert not any(math.isnan(v) for v in got), got                   # the padded row's NaN did not leak
    for k, (a, b) in enumerate(zip(got, want)):
        assert abs(a - b) <= 1e-12 * abs(b), (k, a, b)
    assert psnr.max().item() == pytest.approx(10 * math.log10(4 / 1e-12))     # the identical sample sits at the clamp
