"""`evaluate.Validator`: parity of a validation pass with the CPU oracle at eps = 0, and what a pass must leave untouched.

Parity tolerance: 1e-4 absolute on the two losses, what tests/test_vae_gpu.py::test_forward_matches_oracle_and_golden states for the
same quantities of the same forward (fp16 MFMA operands, fp32 accumulation, against the fp32 CPU reference)."""
import math

import pytest
import torch

from oracle import teacher_ref as T
from oracle import vae_ref as R

pytestmark = pytest.mark.gpu
L = 256


def _vae():
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(latent_dim=L)
    m.load_state_dict(R.closed_form_params(L))           # the weights behind tests/golden/vae_L256_B2.npz
    return m.to("cuda")


def _images(n, salt=0):
    return R.normalise_sprites(R.closed_form_sprites(n, salt))


def test_validation_pass_matches_the_oracle_at_eps_zero():
    from lunaris_orion_amd.evaluate import Validator
    x = _images(2)
    r_ref, mu_ref, lv_ref = R.vae_forward(x, torch.zeros(2, L), R.closed_form_params(L))
    rl_ref, kl_ref = R.vae_losses(r_ref, x, mu_ref, lv_ref)
    res = Validator(_vae()).run([x.cuda()], [2])
    print("validation", res, "oracle", rl_ref.item(), kl_ref.item())
    assert res["n"] == 2
    assert abs(res["val_recon_loss"] - rl_ref.item()) <= 1e-4 and abs(res["val_kl_loss"] - kl_ref.item()) <= 1e-4
    assert res["val_loss"] == pytest.approx(1.0 * res["val_recon_loss"] + 0.1 * res["val_kl_loss"], rel=1e-12)
    assert "val_quality" not in res                       # no teacher
    # PSNR of the oracle's reconstruction, per sample (float64): 1e-4 on an MSE of 0.47 is 1e-3 dB
    mse = ((r_ref - x).double() ** 2).mean(dim=(1, 2, 3))
    psnr = 10 * torch.log10(4 / mse)
    assert abs(res["val_psnr"] - psnr.mean().item()) <= 2e-3 and abs(res["val_psnr_min"] - psnr.min().item()) <= 2e-3
    assert -1.0 <= res["val_ssim"] <= 1.0                 # untrained weights against noise sprites: near 0, either sign


def test_padding_rows_cannot_leak_into_a_pass():
    """At ONE batch size what the padded rows hold is invisible: [a, b, a] and [a, b, NaN] with n_valid = 2 give the same floats, and
    every valid row counts as it does in a full batch ([a, b, a] with n_valid = 3 weighs a twice)."""
    from lunaris_orion_amd.evaluate import Validator
    x = _images(2)
    v = Validator(_vae())
    repeated = torch.cat([x, x[:1]]).cuda()
    poisoned = repeated.clone()
    poisoned[2] = float("nan")
    res = v.run([repeated], [2])
    assert v.run([poisoned], [2]) == res and res["n"] == 2
    full = v.run([repeated], [3])
    assert full["n"] == 3 and full["val_recon_loss"] != res["val_recon_loss"]


def test_batch_padded_to_three_returns_the_floats_of_the_batch_of_two():
    """The two golden images as one batch of 2, and the same call with the batch padded to 3 by repeating its first sample
    (n_valid = 2): identical floats.  A validator computes at one batch size -- here the 2 of its first batch -- because the
    forward's launch plan, and with it the last bits of a sample's sums, depends on the batch size: run on a batch-3 engine the same
    two images give val_recon_loss 0.46837079524993896 against 0.4683706760406494 (measured, MI355X)."""
    from lunaris_orion_amd.evaluate import Validator
    x = _images(2)
    v = Validator(_vae())
    res = v.run([x.cuda()], [2])
    res3 = v.run([torch.cat([x, x[:1]]).cuda()], [2])
    print("batch of 2", res, "padded to 3", res3)
    assert res3 == res
    assert list(v.vae._engines.keys()) == [(2, str(v.vae.flat_parameters().device))]      # no second engine for the odd size


def _steps(stepper, validate_between, teacher=None):
    """Three steps on fixed images, optionally with a validation pass between every two; what must not depend on that."""
    from lunaris_orion_amd.evaluate import Validator
    imgs = [_images(2, salt=s).cuda() for s in (0, 1, 2)]
    held_out = _images(2, salt=9).cuda()
    v = Validator(stepper)
    results = []
    for i, x in enumerate(imgs):
        stepper.step(x, batch_idx=i)
        if validate_between and i < 2:
            results.append(v.run([held_out], [2]))
    stepper.synchronize_parameters()
    torch.cuda.synchronize()
    vae = stepper.vae
    state = {"flat": vae.flat_parameters().clone(), "exp_avg": stepper.exp_avg.clone(), "exp_avg_sq": stepper.exp_avg_sq.clone(),
             "losses": stepper.losses.clone(), "noise_calls": vae.noise_calls, "opt_steps": stepper.opt_steps}
    if teacher is not None:
        state["teacher"] = {k: t.detach().clone() for k, t in teacher.state_dict().items()}
        state["drop_calls"], state["baseline"], state["training"] = teacher.drop_calls, stepper.reward_state.clone(), teacher.training
    return state, results


def _same(a, b, what):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), what
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}[{k}]")
    else:
        assert a == b, what


def test_validation_between_steps_leaves_the_vae_step_unchanged():
    from lunaris_orion_amd.trainer import VAEStepper
    runs = []
    for validate in (False, True):
        torch.manual_seed(11)                              # the noise stream is keyed by the torch seed
        runs.append(_steps(VAEStepper(_vae(), gradient_accumulation_steps=1, pipeline_optimizer=True), validate))
    (plain, _), (mixed, results) = runs
    assert plain["opt_steps"] == 3 and plain["noise_calls"] == 3 and len(results) == 2
    assert results[0] != results[1] and all(r["n"] == 2 for r in results)     # the passes saw different weights
    for k in plain:
        _same(plain[k], mixed[k], k)


def test_validation_between_steps_leaves_the_hybrid_step_and_the_teacher_unchanged():
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from lunaris_orion_amd.trainer import HybridStepper
    runs = []
    for validate in (False, True):
        torch.manual_seed(11)
        t = LunarMoETeacher(dropout_rate=0.1)
        t.load_state_dict(T.closed_form_teacher_state())
        t = t.to("cuda").train()
        stepper = HybridStepper(_vae(), t, gradient_accumulation_steps=1, pipeline_optimizer=True)
        runs.append(_steps(stepper, validate, teacher=t))
    (plain, _), (mixed, results) = runs
    assert plain["training"] is True and mixed["training"] is True
    counters = [int(v) for k, v in plain["teacher"].items() if k.endswith("num_batches_tracked")]
    assert plain["drop_calls"] > 0 and counters and min(counters) > 0          # the steps themselves do move the teacher's state
    assert all(math.isfinite(r["val_quality"]) for r in results)
    for k in plain:
        _same(plain[k], mixed[k], k)


def test_backward_after_a_validation_forward_raises_the_stale_activation_error():
    from lunaris_orion_amd import _lib
    from lunaris_orion_amd.evaluate import Validator
    m = _vae()
    x = _images(2).cuda()
    recon, mu, logvar = m(x)                               # an autograd forward whose activations live in the batch-2 workspace
    Validator(m).run([x], [2])
    with pytest.raises(_lib.LunarisHipError, match="overwritten"):
        recon.sum().backward()
