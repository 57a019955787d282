"""Weight EMA of the VAE in the steppers (`VAEStepper(ema_decay=...)`, `ema_weights()`, `Validator(weights="ema")`).

Every comparison is bitwise: the EMA kernel's three separately rounded fp32 operations against the same three in numpy float32 on
snapshots of the parameters, or the step's own kernels and plan against themselves (a run with the EMA against one without).  Batch 2,
latent 256, the closed-form weights and sprites of tests/test_validation_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import teacher_ref as T
from oracle import vae_ref as R

pytestmark = pytest.mark.gpu
L = 256


def _vae(attention=False):
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(latent_dim=L, attention=attention)
    if attention:
        from tests import attention_ref as A
        m.load_state_dict(A.attention_params(L, gamma=0.5), strict=True)
    else:
        m.load_state_dict(R.closed_form_params(L))
    return m.to("cuda")


def _images(n, salt=0):
    return R.normalise_sprites(R.closed_form_sprites(n, salt))


def _stepper(seed=11, attention=False, **kw):
    from lunaris_orion_amd.trainer import VAEStepper
    torch.manual_seed(seed)                                # the noise stream is keyed by the torch seed
    kw.setdefault("gradient_accumulation_steps", 1)
    return VAEStepper(_vae(attention), **kw)


def _hybrid(seed=11, **kw):
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from lunaris_orion_amd.trainer import HybridStepper
    torch.manual_seed(seed)
    t = LunarMoETeacher(dropout_rate=0.1)
    t.load_state_dict(T.closed_form_teacher_state())
    t = t.to("cuda").train()
    return HybridStepper(_vae(), t, gradient_accumulation_steps=1, **kw), t


def _flat(stepper):
    stepper.synchronize_parameters()
    return stepper.vae.flat_parameters().clone()


def _ema(stepper):
    stepper.synchronize_parameters()
    torch.cuda.synchronize()
    return stepper.ema.clone()


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else t).view(np.uint32)


def _run_and_replay(stepper, n_steps=3):
    """n steps with a snapshot of the parameters after each; returns (the EMA the device holds, the recurrence replayed in numpy float32
    from the snapshots with the schedule the host documents: hostside.ema_decay_at at the step's t, to the power ema_every, 1 - that in
    double, rounded to fp32)."""
    from lunaris_orion_amd.hostside import ema_decay_at, ema_one_minus_decay
    e = _flat(stepper).cpu().numpy()                       # the average starts as a copy of the parameters
    assert np.array_equal(_bits(stepper.ema), _bits(e))
    updates = 0
    for i in range(n_steps):
        stepper.step(_images(2, salt=i).cuda(), batch_idx=i)
        p = _flat(stepper).cpu().numpy()
        if (i + 1) % stepper.ema_every == 0:
            omd = np.float32(ema_one_minus_decay(ema_decay_at(stepper.ema_decay, i, stepper.ema_warmup), stepper.ema_every))
            e = e + (p - e) * omd
            updates += 1
    assert stepper.ema_steps == n_steps and stepper.ema_updates == updates
    return _ema(stepper), e


@pytest.mark.parametrize("kw", [dict(), dict(ema_every=2), dict(ema_warmup=True)], ids=["every1", "every2", "warmup"])
@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "serial"])
def test_ema_follows_the_recurrence(pipelined, kw):
    stepper = _stepper(ema_decay=0.9, pipeline_optimizer=pipelined, **kw)
    got, want = _run_and_replay(stepper)
    assert want.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))
    assert not np.array_equal(_bits(got), _bits(_flat(stepper)))          # it is an average, not a copy
    if kw.get("ema_every") == 2:
        from lunaris_orion_amd.hostside import ema_one_minus_decay
        assert stepper.ema_updates == 1 and np.float32(ema_one_minus_decay(0.9, 2)) == np.float32(1.0 - 0.9 ** 2)


def _steps(stepper, between=None, teacher=None, n=3):
    """Three steps on fixed images, optionally with `between(stepper)` after each of the first two; what must not depend on either that
    or the EMA."""
    for i in range(n):
        stepper.step(_images(2, salt=i).cuda(), batch_idx=i)
        if between is not None and i < n - 1:
            between(stepper)
    stepper.synchronize_parameters()
    torch.cuda.synchronize()
    vae = stepper.vae
    state = {"flat": vae.flat_parameters().clone(), "exp_avg": stepper.exp_avg.clone(), "exp_avg_sq": stepper.exp_avg_sq.clone(),
             "losses": stepper.losses.clone(), "noise_calls": vae.noise_calls, "opt_steps": stepper.opt_steps}
    if teacher is not None:
        state["teacher"] = {k: t.detach().clone() for k, t in teacher.state_dict().items()}
        state["drop_calls"], state["baseline"] = teacher.drop_calls, stepper.reward_state.clone()
    return state


def _same(a, b, what):
    if isinstance(a, torch.Tensor):
        assert torch.equal(a, b), what
    elif isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            _same(a[k], b[k], f"{what}[{k}]")
    else:
        assert a == b, what


@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "serial"])
def test_the_ema_has_no_effect_on_the_step(pipelined):
    plain = _steps(_stepper(pipeline_optimizer=pipelined))
    mixed = _steps(_stepper(pipeline_optimizer=pipelined, ema_decay=0.9))
    assert plain["opt_steps"] == 3 and plain["noise_calls"] == 3
    for k in plain:
        _same(plain[k], mixed[k], k)


def test_pipelined_and_serial_steps_leave_the_same_ema():
    """The ordering test: behind a pipelined step the pass runs on the library's side stream after the deferred AdamW tail, behind a
    serial one on the caller's stream; it must have read the same, final, parameters either way."""
    emas = []
    for pipelined in (True, False):
        stepper = _stepper(pipeline_optimizer=pipelined, ema_decay=0.9)
        _steps(stepper)
        emas.append(_ema(stepper))
    assert torch.equal(emas[0].view(torch.int32), emas[1].view(torch.int32))


@pytest.mark.parametrize("pipelined", [True, False], ids=["pipelined", "serial"])
def test_a_skipped_update_leaves_the_ema_alone(pipelined):
    stepper = _stepper(pipeline_optimizer=pipelined, ema_decay=0.9)
    for i in range(2):
        stepper.step(_images(2, salt=i).cuda(), batch_idx=i)
    before, flat_before = _ema(stepper), _flat(stepper)
    skipped = stepper.metrics()["skipped_steps"]
    bad = _images(2, salt=2)
    bad[0, 1, 5, 7] = float("inf")                         # a non-finite gradient norm: the device skips AdamW, and the EMA pass with it
    stepper.step(bad.cuda(), batch_idx=2)
    after = _ema(stepper)
    assert stepper.metrics()["skipped_steps"] == skipped + 1
    assert torch.equal(_flat(stepper), flat_before)
    assert torch.equal(after.view(torch.int32), before.view(torch.int32))
    assert stepper.ema_steps == 3                          # attempted steps count on the host (hostside.ema_decay_at)


def test_accumulation_updates_the_ema_once_per_window():
    stepper = _stepper(ema_decay=0.9, accumulate_gradients=True, gradient_accumulation_steps=2, pipeline_optimizer=True)
    e = _flat(stepper).cpu().numpy()
    for i in range(4):
        stepper.step(_images(2, salt=i).cuda(), batch_idx=i)
        assert stepper.ema_updates == (i + 1) // 2
        if i % 2 == 1:
            p = _flat(stepper).cpu().numpy()
            e = e + (p - e) * np.float32(1.0 - 0.9)
    assert stepper.opt_steps == 2 and stepper.ema_updates == 2
    assert np.array_equal(_bits(_ema(stepper)), _bits(e))


def test_hybrid_step_keeps_the_ema_and_is_unchanged_by_it():
    from lunaris_orion_amd.hostside import ema_one_minus_decay
    plain_stepper, plain_t = _hybrid(pipeline_optimizer=True)
    plain = _steps(plain_stepper, teacher=plain_t, n=2)
    stepper, t = _hybrid(pipeline_optimizer=True, ema_decay=0.9)
    e = _flat(stepper).cpu().numpy()
    for i in range(2):
        stepper.step(_images(2, salt=i).cuda(), batch_idx=i)
        p = _flat(stepper).cpu().numpy()
        e = e + (p - e) * np.float32(ema_one_minus_decay(0.9, 1))
    assert np.array_equal(_bits(_ema(stepper)), _bits(e))
    mixed = _steps(stepper, teacher=t, n=0)
    assert plain["drop_calls"] > 0 and plain["opt_steps"] == 2
    for k in plain:
        _same(plain[k], mixed[k], k)


def test_attention_model_the_ema_covers_all_86_tensors():
    stepper = _stepper(attention=True, ema_decay=0.9, pipeline_optimizer=True)
    got, want = _run_and_replay(stepper, n_steps=1)
    assert np.array_equal(_bits(got), _bits(want))
    sd, model_sd = stepper.ema_state_dict(), stepper.vae.state_dict()
    assert list(sd.keys()) == list(model_sd.keys()) and len(sd) == 86
    moved = [k for k in sd if not torch.equal(sd[k], model_sd[k].cpu())]
    assert all(sd[k].shape == model_sd[k].shape and sd[k].device.type == "cpu" for k in sd)
    assert any("attn" in k for k in moved), "the attention tensors take part in the average"


def test_ema_validation_equals_a_fresh_model_loaded_with_the_ema_state_dict():
    from lunaris_orion_amd.evaluate import Validator
    from lunaris_orion_amd.vae import LunarisCoreVAE
    stepper = _stepper(ema_decay=0.9, pipeline_optimizer=True)
    _steps(stepper)
    held_out = _images(2, salt=9).cuda()
    ema_res = Validator(stepper, weights="ema").run([held_out], [2])
    live_res = Validator(stepper).run([held_out], [2])
    fresh = LunarisCoreVAE(latent_dim=L)
    fresh.load_state_dict(stepper.ema_state_dict())
    fresh_res = Validator(fresh.to("cuda")).run([held_out], [2])
    print("ema", ema_res, "live", live_res, "fresh", fresh_res)
    assert ema_res.pop("val_weights") == "ema" and "val_weights" not in live_res
    assert ema_res == fresh_res
    assert ema_res["val_loss"] != live_res["val_loss"]
    assert Validator(stepper).run([held_out], [2]) == live_res          # the live weights are back


def test_ema_passes_between_steps_leave_the_step_unchanged():
    """An EMA validation pass and an ema_weights() block with vae.sample(2) after each of the first two steps (pipelined: the swap must wait
    for the side stream, and the restored weights and their re-packed operands must be the live ones bit for bit)."""
    from lunaris_orion_amd.evaluate import Validator
    held_out = _images(2, salt=9).cuda()
    results = []

    def between(stepper):
        results.append(Validator(stepper, weights="ema").run([held_out], [2]))
        rng = torch.cuda.get_rng_state()
        with stepper.ema_weights() as model:
            assert model is stepper.vae
            assert tuple(model.sample(2).shape) == (2, 3, 128, 128)
        torch.cuda.set_rng_state(rng)

    plain = _steps(_stepper(pipeline_optimizer=True))
    mixed_stepper = _stepper(pipeline_optimizer=True, ema_decay=0.9)
    mixed = _steps(mixed_stepper, between)
    assert len(results) == 2 and results[0] != results[1]
    for k in plain:
        _same(plain[k], mixed[k], k)
    # ... and the average itself went through the two passes untouched: the run without them holds the same one
    untouched = _stepper(pipeline_optimizer=True, ema_decay=0.9)
    _steps(untouched)
    assert torch.equal(_ema(mixed_stepper).view(torch.int32), _ema(untouched).view(torch.int32))


def test_step_inside_ema_weights_raises_and_the_block_still_restores():
    stepper = _stepper(ema_decay=0.9)
    x = _images(2).cuda()
    stepper.step(x, batch_idx=0)
    live = _flat(stepper)
    with stepper.ema_weights():
        assert torch.equal(stepper.vae.flat_parameters(), stepper.ema)
        with pytest.raises(RuntimeError, match="ema_weights"):
            stepper.step(x, batch_idx=1)
        with pytest.raises(RuntimeError, match="nest"):
            with stepper.ema_weights():
                pass
    assert torch.equal(_flat(stepper), live)
    stepper.step(x, batch_idx=1)                          # and training goes on
    assert stepper.opt_steps == 2


def test_no_ema_means_no_buffer_and_clear_errors():
    from lunaris_orion_amd.evaluate import Validator
    stepper = _stepper()
    assert stepper.ema is None and stepper.ema_decay == 0.0
    stepper.step(_images(2).cuda(), batch_idx=0)
    assert stepper.ema is None and stepper.ema_updates == 0
    with pytest.raises(ValueError, match="ema"):
        Validator(stepper, weights="ema")
    with pytest.raises(ValueError, match="ema"):
        Validator(stepper.vae, weights="ema")
    with pytest.raises(RuntimeError, match="ema_decay"):
        with stepper.ema_weights():
            pass
    with pytest.raises(RuntimeError, match="ema_decay"):
        stepper.ema_state_dict()
    for bad in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=0.5, ema_every=0)):
        with pytest.raises(ValueError, match="ema_"):
            _stepper(**bad)
