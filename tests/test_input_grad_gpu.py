"""Gradients with respect to the input images (train_hybrid.py:845: ``images.requires_grad_(True)`` before ``self.vae(images)``) and
through the teacher used as a differentiable reward, against autograd of the CPU oracle (oracle/vae_ref.py, oracle/teacher_ref.py) on
closed-form parameters and sprites.

  * the kernel alone (lo_image_dgrad_op) against ``torch.nn.grad.conv2d_input`` in fp64 on the same fp16 dy: only the summation order
    differs, so the bound is 1e-5;
  * the VAE's encoder, the whole VAE with the reference's loss (parameters live and frozen), the same under autocast + GradScaler,
    ``decode(z)``: the bounds of tests/test_vae_gpu.py (3e-2 relative L2, fp16 activation gradients);
  * the teacher in train mode and the teacher-as-reward chain.  The parameter gradients are the full backward's (bitwise); x.grad is the
    data gradient of the same pass, which ``<x, x.grad> == <W, dW>`` of feature_extractor.conv1.0 pins to 1e-6.  Against the oracle
    x.grad is per-pixel and carries the full backward's unbiased fp16 noise (LeakyReLU's kink, tests/test_teacher_fullgrad_gpu.py)
    without the averaging a weight gradient gets: measured 5.0 % / 6.4 % relative L2 (dropout 0.1 / 0), cosine 0.9987 / 0.9980, norm
    ratio 1.0004 / 1.0002, and 2.4-2.7 % / 0.6-0.8 % after 4x4 / 16x16 average pooling.  Bounds: 8e-2, cosine >= 0.997, norm within
    1 %, 16x16-pooled 2e-2;
  * what must not move: outputs and parameter gradients with and without an input that requires grad, run-to-run bitwise x.grad, the
    eval-mode teacher.
"""
import warnings

import pytest
import torch

from oracle import dropout_ref as D
from oracle import teacher_ref as T
from oracle import vae_ref as R

pytestmark = pytest.mark.gpu
L = 256
DROP_SEED, DROP_P, QW = 0x5EEDD209C0FFEE11, 0.1, 0.5


def _rel(a, b):
    return (a.double() - b.double()).norm().item() / (b.double().norm().item() + 1e-30)


def _vae(frozen=False):
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(latent_dim=L)
    m.load_state_dict(R.closed_form_params(L))
    m = m.to("cuda")
    if frozen:
        m.requires_grad_(False)
    return m


def _teacher(drop, full_backward=False):
    from lunaris_orion_amd.teacher import LunarMoETeacher
    t = LunarMoETeacher(dropout_rate=DROP_P if drop else 0.0, full_backward=full_backward)
    t.load_state_dict(T.closed_form_teacher_state())
    t = t.to("cuda").train()
    t.set_dropout_stream(DROP_SEED, exact_next=True)
    return t


def _x(B=2):
    return R.normalise_sprites(R.closed_form_sprites(B))


def _oracle_params(live=True):
    P = R.closed_form_params(L)
    return {k: v.clone().requires_grad_(live) for k, v in P.items()}


def _assert_teacher_input_grad_close(got, ref, what):
    """x.grad of the teacher's full backward against the oracle (see the module docstring for the measured noise)."""
    pooled = _rel(torch.nn.functional.avg_pool2d(got.double(), 16), torch.nn.functional.avg_pool2d(ref.double(), 16))
    assert pooled <= 2e-2, (what, pooled)
    got, ref = got.double().flatten(), ref.double().flatten()
    assert _rel(got, ref) <= 8e-2, (what, _rel(got, ref))
    cos = torch.dot(got, ref).item() / (got.norm().item() * ref.norm().item())
    assert cos >= 0.997, (what, cos)
    assert abs(got.norm().item() / ref.norm().item() - 1.0) <= 1e-2, (what, got.norm().item(), ref.norm().item())


def _assert_first_conv_identity(x, dx, w, dw):
    """<x, dx> == <W, dW> for a bias-carrying conv whose input gradient and weight gradient come from the same dy (both equal
    <conv(x, W), dy>): pins the images' gradient to the weight gradient the parameter tests already check."""
    x, dx, w, dw = (t.detach().double().cpu() for t in (x, dx, w, dw))
    lhs, rhs = (x * dx).sum().item(), (w * dw).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * (x.abs() * dx.abs()).sum().item(), (lhs, rhs)


# ---- 1. the kernel through the raw ABI ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride,cout", [(1, 32), (2, 64)])
@pytest.mark.parametrize("B", [1, 3, 64])
def test_image_dgrad_kernel_matches_conv2d_input(stride, cout, B):
    _image_dgrad_kernel(stride, cout, B)


@pytest.mark.parametrize("stride,cout", [(1, 32), (2, 64)])
def test_image_dgrad_kernel_aligned16(stride, cout):
    """Every pointer at (a multiple of 256 B) + 16 B: the alignment include/lunaris_hip.h promises."""
    _image_dgrad_kernel(stride, cout, 3, skew=16)


def _image_dgrad_kernel(stride, cout, B, skew=0):
    from lunaris_orion_amd import _lib
    from tests.guarded import check_guards, gin, guarded
    g = torch.Generator().manual_seed(1000 * stride + B)
    ho = 128 // stride
    dy = torch.randn(B, ho, ho, cout, generator=g).half()          # NHWC, the backward's fp16 layout
    w = torch.randn(cout, 3, 3, 3, generator=g) * 0.2
    scale = 2.0 ** -3
    dyc, wc = gin(dy, skew), gin(w, skew)                                       # guard-banded, exactly the header's sizes (tests/guarded.py)
    dx = guarded((B, 3, 128, 128), torch.float32, "out", skew)            # pre-filled with NaN: every element must be written
    _lib.check(_lib.lib.lo_image_dgrad_op(dyc.data_ptr(), cout, stride, wc.data_ptr(), B, scale, dx.data_ptr(), _lib.stream_ptr()),
               "lo_image_dgrad_op")
    torch.cuda.synchronize()
    ref = torch.nn.grad.conv2d_input((B, 3, 128, 128), w.double(), dy.double().permute(0, 3, 1, 2), stride=stride, padding=1) * scale
    got = dx.cpu().double()
    assert torch.isfinite(got).all()
    assert _rel(got, ref) <= 1e-5, _rel(got, ref)
    # border rows / columns (the padding of the forward) and the last sample on their own
    for a, b in ((got[:, :, 0], ref[:, :, 0]), (got[:, :, -1], ref[:, :, -1]), (got[:, :, :, 0], ref[:, :, :, 0]),
                 (got[:, :, :, -1], ref[:, :, :, -1]), (got[-1], ref[-1])):
        assert _rel(a, b) <= 1e-5, _rel(a, b)
    # deterministic: the same call again gives the same bits
    dx2 = guarded((B, 3, 128, 128), torch.float32, "out", skew)
    _lib.check(_lib.lib.lo_image_dgrad_op(dyc.data_ptr(), cout, stride, wc.data_ptr(), B, scale, dx2.data_ptr(), _lib.stream_ptr()),
               "lo_image_dgrad_op")
    assert torch.equal(dx, dx2)
    check_guards(dyc, wc, dx, dx2)


def test_image_dgrad_rejects_shapes_it_is_not_built_for():
    from lunaris_orion_amd import _lib
    buf = torch.zeros(16, device="cuda")
    assert _lib.lib.lo_image_dgrad_op(buf.data_ptr(), 64, 1, buf.data_ptr(), 1, 1.0, buf.data_ptr(), _lib.stream_ptr()) == -1
    assert _lib.lib.lo_image_dgrad_op(buf.data_ptr(), 32, 2, buf.data_ptr(), 1, 1.0, buf.data_ptr(), _lib.stream_ptr()) == -1


# ---- 2. the encoder alone -------------------------------------------------------------------------------------------------------
def test_encoder_input_grad_matches_the_oracle():
    vae = _vae()
    x = _x(2)
    xg = x.cuda().requires_grad_()
    mu, logvar, skips = vae.encoder(xg)
    g = torch.Generator().manual_seed(7)
    ups = [torch.randn(t.shape, generator=g) for t in (mu, logvar, *skips)]
    torch.autograd.backward([mu, logvar, *skips], [u.cuda() for u in ups])
    assert xg.grad is not None
    xr = x.clone().requires_grad_()
    omu, olv, osk = R.encoder_forward(xr, _oracle_params(False))
    torch.autograd.backward([omu, olv, *osk], ups)
    assert _rel(xg.grad.cpu(), xr.grad) <= 3e-2, _rel(xg.grad.cpu(), xr.grad)
    w = vae.encoder.down1[0].weight
    _assert_first_conv_identity(xg, xg.grad, w, w.grad)


def _vae_step(vae, x, eps, amp=False):
    """vae(images) + the reference's loss (train_hybrid.py:850-862) -> backward; returns (x.grad, recon)."""
    xg = x.cuda().requires_grad_()
    if amp:
        scaler = torch.amp.GradScaler("cuda")
        with torch.autocast("cuda", dtype=torch.float16):
            recon, mu, logvar = vae(xg, eps.cuda())
            rl, kl = R.vae_losses(recon, xg, mu, logvar)
            loss = rl + 0.1 * kl
        scaler.scale(loss).backward()
        return xg.grad / scaler.get_scale(), recon
    recon, mu, logvar = vae(xg, eps.cuda())
    rl, kl = R.vae_losses(recon, xg, mu, logvar)
    (rl + 0.1 * kl).backward()
    return xg.grad, recon


# ---- 3. the whole VAE, the reference's loss ------------------------------------------------------------------------------------
@pytest.mark.parametrize("frozen", [False, True])
def test_vae_input_grad_with_the_reference_loss(frozen):
    x, eps = _x(2), R.closed_form_eps(2, L)
    vae = _vae(frozen)
    gx, recon = _vae_step(vae, x, eps)
    assert gx is not None
    P = _oracle_params(not frozen)
    xr = x.clone().requires_grad_()
    orec, omu, olv = R.vae_forward(xr, eps, P)
    rl, kl = R.vae_losses(orec, xr, omu, olv)
    (rl + 0.1 * kl).backward()
    assert _rel(gx.cpu(), xr.grad) <= 3e-2, _rel(gx.cpu(), xr.grad)
    # the encoder's share alone (x.grad minus the direct term of mse_loss(recon, x), d/dx = 2 (x - recon) / N)
    n = x.numel()
    enc_gpu = gx.cpu() - 2.0 * (x - recon.detach().cpu()) / n
    enc_ref = xr.grad - 2.0 * (x - orec.detach()) / n
    assert _rel(enc_gpu, enc_ref) <= 3e-2, _rel(enc_gpu, enc_ref)
    if frozen:
        assert all(p.grad is None for p in vae.parameters())
    else:
        for k, p in vae.named_parameters():
            assert p.grad is not None, k
        for k in ("encoder.down1.0.weight", "decoder.final_conv.weight"):
            assert _rel(dict(vae.named_parameters())[k].grad.cpu(), P[k].grad) <= 3e-2, k


# ---- 4. autocast + GradScaler ---------------------------------------------------------------------------------------------------
def test_vae_input_grad_under_autocast_and_gradscaler():
    x, eps = _x(2), R.closed_form_eps(2, L)
    g32, _ = _vae_step(_vae(), x, eps)
    gamp, _ = _vae_step(_vae(), x, eps, amp=True)
    assert _rel(gamp.cpu(), g32.cpu()) <= 1e-4, _rel(gamp.cpu(), g32.cpu())


# ---- 5. the teacher in train mode -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("drop", [False, True])
def test_teacher_input_grad_in_train_mode(drop):
    B = 2
    x = _x(B)
    t = _teacher(drop)                                  # full_backward=False: an input that requires grad takes the full backward
    xg = x.cuda().requires_grad_()
    out = t(xg)
    (QW * -torch.mean(out["quality_scores"])).backward()
    assert xg.grad is not None
    xr = x.clone().requires_grad_()
    masks = D.TeacherMasks(DROP_SEED, DROP_P, B) if drop else None
    oo, _ = T.teacher_forward(xr, T.closed_form_teacher_state(), training=True, masks=masks)
    (QW * -torch.mean(oo["quality_scores"])).backward()
    _assert_teacher_input_grad_close(xg.grad.cpu(), xr.grad, "x.grad")
    w = t.feature_extractor.conv1[0].weight
    _assert_first_conv_identity(xg, xg.grad, w, w.grad)
    # the parameter gradients are those of full_backward=True on the same call
    tf = _teacher(drop, full_backward=True)
    outf = tf(x.cuda())
    (QW * -torch.mean(outf["quality_scores"])).backward()
    assert torch.equal(out["quality_scores"], outf["quality_scores"])
    live = 0
    for (k, p), (kf, pf) in zip(t.named_parameters(), tf.named_parameters()):
        assert k == kf
        assert (p.grad is None) == (pf.grad is None), k
        if pf.grad is not None:
            live += 1
            assert torch.equal(p.grad, pf.grad), k
    assert live > 200


# ---- 5b. the same x.grad against the fp16-rounding oracle ------------------------------------------------------------------------
INPUT_GRAD_ROUNDED_BOUND = {"full": 3e-2, "pooled16": 4e-3}      # measured, see the table in tests/test_teacher_fullgrad_gpu.py


@pytest.mark.parametrize("drop", [False, True])
def test_teacher_input_grad_against_the_fp16_rounding_oracle(drop):
    """lo_teacher_full_backward_dx against x.grad of the oracle that rounds to fp16 where the plain-form forward does
    (oracle/teacher_ref.py, act_dtype): same structure as _assert_teacher_input_grad_close, bounds from the measurement."""
    from tests.test_teacher_fullgrad_gpu import _oracle_extras
    B = 2
    x = _x(B)
    t = _teacher(drop)
    xg = x.cuda().requires_grad_()
    (QW * -torch.mean(t(xg)["quality_scores"])).backward()
    got = xg.grad.cpu()
    ref, ref32 = _oracle_extras(x, drop, act_dtype=torch.float16)["x_grad"], _oracle_extras(x, drop)["x_grad"]
    pool = lambda a: torch.nn.functional.avg_pool2d(a.double(), 16)
    full, pooled = _rel(got, ref), _rel(pool(got), pool(ref))
    print(f"x.grad against the rounding oracle: {full:.4f}, 16x16-pooled {pooled:.4f}  (fp32 oracle: {_rel(got, ref32):.4f}, {_rel(pool(got), pool(ref32)):.4f})")
    assert full <= INPUT_GRAD_ROUNDED_BOUND["full"], full
    assert pooled <= INPUT_GRAD_ROUNDED_BOUND["pooled16"], pooled
    g, r = got.double().flatten(), ref.double().flatten()
    cos = torch.dot(g, r).item() / (g.norm().item() * r.norm().item())
    assert cos >= 1.0 - 0.5 * INPUT_GRAD_ROUNDED_BOUND["full"] ** 2 - 1e-6, cos       # what a deviation of that size can do to the direction
    assert abs(g.norm().item() / r.norm().item() - 1.0) <= 1e-2, (g.norm().item(), r.norm().item())


# ---- 6. the teacher as a differentiable reward ----------------------------------------------------------------------------------
def test_teacher_as_a_differentiable_reward_reaches_the_vae_and_the_images():
    x, eps = _x(2), R.closed_form_eps(2, L)
    vae = _vae()
    t = _teacher(False)
    t.requires_grad_(False)                              # a fixed reward model: only its input gradient is wanted
    xg = x.cuda().requires_grad_()
    recon, mu, logvar = vae(xg, eps.cuda())
    rl, kl = R.vae_losses(recon, xg, mu, logvar)
    q = t(recon)["quality_scores"]
    (rl + 0.1 * kl - 0.5 * q.mean()).backward()

    def oracle(with_teacher):
        P = _oracle_params(True)
        xr = x.clone().requires_grad_()
        orec, omu, olv = R.vae_forward(xr, eps, P)
        orl, okl = R.vae_losses(orec, xr, omu, olv)
        loss = orl + 0.1 * okl
        if with_teacher:
            oo, _ = T.teacher_forward(orec, T.closed_form_teacher_state(), training=True)
            loss = loss - 0.5 * oo["quality_scores"].mean()
        loss.backward()
        return xr.grad, torch.cat([P[k].grad.flatten() for k in P])

    gx_ref, gp_ref = oracle(True)
    gx_no, gp_no = oracle(False)
    gp = torch.cat([p.grad.flatten().cpu() for p in vae.parameters()])
    err_x, err_p = _rel(xg.grad.cpu(), gx_ref), _rel(gp, gp_ref)
    assert err_x <= 3e-2 and err_p <= 3e-2, (err_x, err_p)
    # the teacher's share is visibly there: the result is far closer to the oracle with the reward than to the one without it
    assert _rel(xg.grad.cpu(), gx_no) >= max(2 * err_x, 1e-3), (_rel(xg.grad.cpu(), gx_no), err_x)
    assert _rel(gp, gp_no) >= max(2 * err_p, 1e-3), (_rel(gp, gp_no), err_p)


# ---- 7. decode(z) ---------------------------------------------------------------------------------------------------------------
def test_decode_z_grad_matches_the_oracle():
    vae = _vae()
    z = R.closed_form_eps(2, L)
    zg = z.cuda().requires_grad_()
    recon = vae.decode(zg)
    up = torch.randn(recon.shape, generator=torch.Generator().manual_seed(3))
    recon.backward(up.cuda())
    assert zg.grad is not None
    zr = z.clone().requires_grad_()
    R.decoder_forward(zr, [], _oracle_params(False)).backward(up)
    assert _rel(zg.grad.cpu(), zr.grad) <= 3e-2, _rel(zg.grad.cpu(), zr.grad)
    with torch.no_grad():                                 # the plain decode is the same function
        assert (vae.decode(z.cuda()) - recon.detach()).abs().max().item() <= 1e-3


# ---- 8. what does not move ------------------------------------------------------------------------------------------------------
def _vae_run(x_requires_grad):
    vae = _vae()
    x, eps = _x(2), R.closed_form_eps(2, L)
    xc = x.cuda().requires_grad_(x_requires_grad)
    recon, mu, logvar = vae(xc, eps.cuda())
    rl, kl = R.vae_losses(recon, xc.detach(), mu, logvar)
    (rl + 0.1 * kl).backward()
    return (recon, mu, logvar), [p.grad.clone() for p in vae.parameters()], xc.grad


def test_vae_outputs_and_parameter_grads_do_not_depend_on_the_input_requiring_grad():
    o0, g0, dx0 = _vae_run(False)
    o1, g1, dx1 = _vae_run(True)
    _, _, dx2 = _vae_run(True)
    assert dx0 is None and dx1 is not None
    for a, b in zip(o0, o1):
        assert torch.equal(a, b)
    for a, b in zip(g0, g1):
        assert torch.equal(a, b)
    assert torch.equal(dx1, dx2)                          # run to run, bit for bit


def _teacher_run(x_requires_grad):
    t = _teacher(True, full_backward=True)
    xc = _x(2).cuda().requires_grad_(x_requires_grad)
    out = t(xc)
    (QW * -torch.mean(out["quality_scores"])).backward()
    return out, [None if p.grad is None else p.grad.clone() for p in t.parameters()], xc.grad


def test_teacher_full_backward_outputs_and_grads_do_not_depend_on_the_input_requiring_grad():
    o0, g0, dx0 = _teacher_run(False)
    o1, g1, dx1 = _teacher_run(True)
    _, _, dx2 = _teacher_run(True)
    assert dx0 is None and dx1 is not None
    for k in ("quality_scores", "expert_weights", "style_embedding", "prompt_embedding", "semantic_score"):
        assert torch.equal(o0[k], o1[k]), k
    for a, b in zip(g0, g1):
        assert (a is None and b is None) or torch.equal(a, b)
    assert torch.equal(dx1, dx2)


def test_teacher_in_eval_mode_warns_and_keeps_its_outputs():
    t = _teacher(True)
    t.eval()
    x = _x(2).cuda()
    ref = t(x)
    xg = x.clone().requires_grad_()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = t(xg)
    assert any(issubclass(w.category, UserWarning) and "eval mode" in str(w.message) for w in rec), [str(w.message) for w in rec]
    for k in ("quality_scores", "expert_weights", "style_embedding", "prompt_embedding", "semantic_score"):
        assert torch.equal(out[k].detach(), ref[k]), k
    out["quality_scores"].mean().backward()               # the gate / quality heads as before; the images get nothing
    assert xg.grad is None
