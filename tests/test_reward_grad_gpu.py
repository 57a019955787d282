"""The hybrid step with ``reward_grad_weight`` (lambda): the VAE trained through the frozen, eval-mode teacher's quality score,

    vae_loss = (recon_weight * MSE + kl_weight * KL - mean_advantage * MSE - lambda * mean(q_eval)) / accum,
    q_eval   = quality_scores [B, 4] of the teacher in eval mode on recon (not detached; the teacher's parameters are constants).

Oracle: autograd of ``R.vae_forward`` -> ``T.teacher_forward(recon, S, training=False[, act_dtype=torch.float16])`` on the CPU, one
graph for every case (the objective is linear in its three parts: the default objective's gradient, the reward's with the fp32
teacher and the reward's with the fp16-rounding teacher).  B = 2, latent 256, closed-form parameters / sprites / eps and the closed-form
teacher state (the helpers of tests/test_input_grad_gpu.py and tests/test_teacher_eval_grad_gpu.py, restated).  The state S of the
eval call is the one the eval pass finds: the closed-form state with its running statistics advanced by the step's two train-mode
calls (oracle train-mode forwards on images and on recon, dropout 0 in these cases).  With the closed-form statistics themselves the
native gradient is a different function's (cosine -0.63 to that oracle, measured).

lambda = 50: at 0.5 the reward is 1.2 % of the default objective's gradient (below the 3e-2 parity bound: a mixed test would pass
without the feature); at 50 the two parts have the same order of size (3.4 against 2.9 at the closed-form statistics).

Bounds.  All 72 gradients, global relative L2 3e-2, cosine >= 0.999, norm within 1 %; per tensor (oracle norm >= 1e-3 of the largest)
6e-2 against the oracle with the fp16-rounding teacher and 8e-2 against the fp32 one: composed from the project's own -- 3e-2 per VAE
tensor (tests/test_vae_gpu.py), 3e-2 / 8e-2 for x.grad of the eval teacher (tests/test_teacher_eval_grad_gpu.py); the VAE backward is
linear in its seed, so the two errors add.  The seeded kernel alone: 1e-5 relative L2 against fp64, the bound of the un-seeded op
(only the summation order differs).  Measured values: the docstring of each test.
"""
import ctypes as C
import os

import pytest
import torch

from oracle import teacher_ref as T
from oracle import vae_ref as R

pytestmark = pytest.mark.gpu
L, B, LAM = 256, 2, 50.0
DROP_SEED = 0x5EEDD209C0FFEE11


def _rel(a, b):
    return (a.double() - b.double()).norm().item() / (b.double().norm().item() + 1e-30)


def _x(n=B):
    return R.normalise_sprites(R.closed_form_sprites(n))


def _eps(salt=0):
    return R.closed_form_eps(B, L, salt=salt)


# ---- the oracle, once -----------------------------------------------------------------------------------------------------------
_ORACLE = {}


def _oracle():
    """{"names", "default", "reward32", "reward16": lists of 72 gradients (reward*: of -LAM * mean(q_eval)), "recon_loss", "kl_loss",
    "q32", "q16": mean(q_eval)} -- read-only."""
    if not _ORACLE:
        P = {k: v.clone().requires_grad_(True) for k, v in R.closed_form_params(L).items()}
        x = _x()
        recon, mu, logvar = R.vae_forward(x, _eps(), P)
        # "at its running statistics": the ones the eval pass finds -- the closed-form state after the step's two train-mode calls
        # (teacher(images), whose result is dead, and teacher(recon)) have moved them; no dropout in the oracle cases, so no masks
        S = dict(T.closed_form_teacher_state())
        with torch.no_grad():
            for seen in (x, recon.detach()):
                S.update(T.teacher_forward(seen, S, training=True)[1])
        rl, kl = R.vae_losses(recon, x, mu, logvar)
        q32 = T.teacher_forward(recon, S, training=False)[0]["quality_scores"].mean()
        q16 = T.teacher_forward(recon, S, training=False, act_dtype=torch.float16)[0]["quality_scores"].mean()
        names, params = list(P.keys()), list(P.values())
        grad = lambda loss: [g.detach() for g in torch.autograd.grad(loss, params, retain_graph=True)]
        _ORACLE.update(names=names, default=grad(R.vae_objective(rl, kl)[0]), reward32=grad(-LAM * q32), reward16=grad(-LAM * q16),
                       recon_loss=rl.item(), kl_loss=kl.item(), q32=q32.item(), q16=q16.item())
    return _ORACLE


def _sum(a, b):
    return [u + v for u, v in zip(a, b)]


# ---- native -----------------------------------------------------------------------------------------------------------------------
def _stepper(lam=None, full=False, accum=1, dropout=0.1, **kw):
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from lunaris_orion_amd.trainer import HybridStepper
    from lunaris_orion_amd.vae import LunarisCoreVAE
    vae = LunarisCoreVAE(L)
    vae.load_state_dict(R.closed_form_params(L))
    vae = vae.to("cuda")
    t = LunarMoETeacher(dropout_rate=dropout)               # 0.1 like the reference: the train-mode calls draw masks
    t.load_state_dict(T.closed_form_teacher_state())
    t = t.to("cuda").train()
    t.set_dropout_stream(DROP_SEED)
    if lam is not None:
        kw["reward_grad_weight"] = lam
    return HybridStepper(vae, t, gradient_accumulation_steps=accum, teacher_full_backward=full, **kw)


def _grads(hs):
    return [g.detach().cpu().clone() for g in hs.parameter_grads()]


def _global(got, ref):
    num = sum(((g.double() - r.double()) ** 2).sum().item() for g, r in zip(got, ref))
    den = sum((r.double() ** 2).sum().item() for r in ref)
    return (num / den) ** 0.5


def _cos_norm(got, ref):
    dot = sum((g.double() * r.double()).sum().item() for g, r in zip(got, ref))
    ng = sum((g.double() ** 2).sum().item() for g in got) ** 0.5
    nr = sum((r.double() ** 2).sum().item() for r in ref) ** 0.5
    return dot / (ng * nr), ng / nr


_NATIVE = {}


def _native(kind):
    """(gradients, metrics) of ONE step at lambda = 50, reward_scale = 0: "pure" (recon_weight = kl_weight = 0) or "mixed" (defaults)."""
    if kind not in _NATIVE:
        kw = {"recon_weight": 0.0, "kl_weight": 0.0} if kind == "pure" else {}
        hs = _stepper(LAM, reward_scale=0.0, dropout=0.0, **kw)
        hs.step(_x().cuda(), 0, _eps().cuda())
        m = hs.metrics()
        assert m["grads_finite"] == 1.0
        _NATIVE[kind] = (_grads(hs), m)
    return _NATIVE[kind]


# ---- 1. the seeded kernel through the raw ABI -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
def test_seeded_image_dgrad_op(n):
    """Measured on the MI355X: 1.05e-7 (B = 1) and 1.03e-7 (B = 3) relative L2 against fp64."""
    from lunaris_orion_amd import _lib
    from tests.guarded import check_guards, gin, guarded
    lib, st = _lib.lib, _lib.stream_ptr()
    g = torch.Generator().manual_seed(4100 + n)
    dy = torch.randn(n, 128, 128, 32, generator=g).half()
    w = torch.randn(32, 3, 3, 3, generator=g) * 0.2
    recon, target = torch.tanh(torch.randn(n, 3, 128, 128, generator=g)), torch.rand(n, 3, 128, 128, generator=g) * 2 - 1
    scale, c = 2.0 ** -3, 0.37
    dyc, wc, rc, tc = gin(dy), gin(w), gin(recon), gin(target)
    plain = guarded((n, 3, 128, 128), torch.float32, "out")
    _lib.check(lib.lo_image_dgrad_op(dyc.data_ptr(), 32, 1, wc.data_ptr(), n, scale, plain.data_ptr(), st), "lo_image_dgrad_op")
    zero, some = gin(torch.zeros(1)), gin(torch.full((1,), c))
    dx0 = guarded((n, 3, 128, 128), torch.float32, "out")             # NaN-filled: every element must be written
    dxc = guarded((n, 3, 128, 128), torch.float32, "out")
    for coef, out in ((zero, dx0), (some, dxc)):
        _lib.check(lib.lo_image_dgrad_seed_op(dyc.data_ptr(), 32, 1, wc.data_ptr(), n, scale, coef.data_ptr(), rc.data_ptr(), tc.data_ptr(),
                                              out.data_ptr(), st), "lo_image_dgrad_seed_op")
    torch.cuda.synchronize()
    check_guards(dyc, wc, rc, tc, plain, zero, some, dx0, dxc)
    assert torch.equal(dx0, plain)                                             # scalar 0: the bits of the un-seeded op
    ref = (torch.nn.grad.conv2d_input((n, 3, 128, 128), w.double(), dy.double().permute(0, 3, 1, 2), stride=1, padding=1) * scale
           + float(torch.tensor(c)) * (recon.double() - target.double()))
    got = dxc.cpu().double()
    assert torch.isfinite(got).all()
    print("seeded op, relative L2 against fp64:", _rel(got, ref))
    assert _rel(got, ref) <= 1e-5, _rel(got, ref)
    for a, b in ((got[:, :, 0], ref[:, :, 0]), (got[:, :, -1], ref[:, :, -1]), (got[:, :, :, 0], ref[:, :, :, 0]),
                 (got[:, :, :, -1], ref[:, :, :, -1]), (got[-1], ref[-1])):
        assert _rel(a, b) <= 1e-5, _rel(a, b)
    # rejected shapes still return an error: the seeded form exists for (stride 1, 32 channels) only, and needs all three operands
    buf = torch.zeros(16, device="cuda")
    p = buf.data_ptr()
    assert lib.lo_image_dgrad_seed_op(p, 64, 2, p, 1, 1.0, p, p, p, p, st) == -1
    assert lib.lo_image_dgrad_seed_op(p, 64, 1, p, 1, 1.0, p, p, p, p, st) == -1
    assert lib.lo_image_dgrad_seed_op(p, 32, 1, p, 1, 1.0, None, p, p, p, st) == -1
    assert lib.lo_image_dgrad_seed_op(p, 32, 1, p, 0, 1.0, p, p, p, p, st) == -1


# ---- 2. pure reward -----------------------------------------------------------------------------------------------------------------
def test_pure_reward_gradients_against_both_oracles():
    """recon_weight = kl_weight = reward_scale = 0, lambda = 50: every gradient is the reward's.  Measured on the MI355X: rounding
    oracle global 2.18e-3, cosine 0.999998, norm ratio 0.99962, worst tensor 4.18e-2 (encoder.fc_logvar.weight; decoder.fc.weight
    4.02e-2 next); fp32 oracle 2.22e-3, 0.999998, 0.99991, worst 4.43e-2 (encoder.fc_logvar.weight); 15 tensors left out with 9.1e-7
    of the squared norm.  No starting bound exceeded."""
    o = _oracle()
    got, m = _native("pure")
    assert len(got) == len(o["names"]) == 72
    for ref_key, per_tensor in (("reward16", 6e-2), ("reward32", 8e-2)):
        ref = o[ref_key]
        glob = _global(got, ref)
        cos, ratio = _cos_norm(got, ref)
        norms = [r.double().norm().item() for r in ref]
        big = max(norms)
        tot2 = sum(v * v for v in norms)
        left_out = [k for k, v in zip(o["names"], norms) if v < 1e-3 * big]
        left2 = sum(v * v for v in norms if v < 1e-3 * big)
        worst = sorted(((_rel(g, r), k) for g, r, k, v in zip(got, ref, o["names"], norms) if v >= 1e-3 * big), reverse=True)
        print(f"pure reward against {ref_key}: global {glob:.4e}, cosine {cos:.6f}, norm ratio {ratio:.5f}, left out {len(left_out)} "
              f"tensors with {left2 / tot2:.2e} of the squared norm, worst tensors {[(k, f'{e:.3e}') for e, k in worst[:4]]}")
        assert glob <= 3e-2, (ref_key, glob)
        assert cos >= 0.999 and abs(ratio - 1.0) <= 1e-2, (ref_key, cos, ratio)
        assert len(left_out) <= 16 and left2 <= 1e-5 * tot2, (ref_key, left_out, left2 / tot2)
        bad = [(k, e) for e, k in worst if e > per_tensor]
        assert not bad, (ref_key, bad)
    assert abs(m["eval_quality"] - o["q32"]) <= 2e-3 and abs(m["reward_grad_loss"] + LAM * m["eval_quality"]) <= 1e-5 * LAM


# ---- 3. mixed objective ---------------------------------------------------------------------------------------------------------
def test_mixed_objective_needs_the_reward_term():
    """Defaults, reward_scale = 0, lambda = 50: the gradient is the oracle's WITH the term, and ten errors away from the one without.
    Measured on the MI355X: 1.81e-3 against the oracle with the term, 1.44 against the one without; eval_quality 0.497861 (oracle
    0.497863, rounding oracle 0.497864)."""
    o = _oracle()
    got, m = _native("mixed")
    err = _global(got, _sum(o["default"], o["reward32"]))
    away = _global(got, o["default"])
    print(f"mixed: global {err:.4e} against the oracle with the term, {away:.4e} against the one without; eval_quality {m['eval_quality']:.6f} "
          f"(oracle {o['q32']:.6f}, rounding oracle {o['q16']:.6f})")
    assert err <= 3e-2, err
    assert away >= 10 * err, (away, err)
    assert abs(m["recon_loss"] - o["recon_loss"]) <= 1e-4 and abs(m["kl_loss"] - o["kl_loss"]) <= 1e-4
    assert abs(m["eval_quality"] - o["q32"]) <= 2e-3
    formula = 1.0 * m["recon_loss"] + 0.1 * m["kl_loss"] + m["pg_loss"] - LAM * m["eval_quality"]
    assert abs(m["vae_loss"] - formula) <= 1e-5 * max(1.0, abs(formula)), (m["vae_loss"], formula)
    assert abs(m["total_loss"] - (m["vae_loss"] + m["teacher_loss"])) <= 1e-6 * max(1.0, abs(m["vae_loss"]))


# ---- 4. what must not move ------------------------------------------------------------------------------------------------------
def _snapshot(hs):
    torch.cuda.synchronize()
    return {"params": hs.vae._flat.clone(), "grads": hs.flat_grads().clone(), "t_flat": hs.teacher._flat.clone(), "t_grads": hs.t_grads.clone(),
            "drop_calls": hs.teacher.drop_calls, "nbt": hs.teacher._nbt.clone()}


def test_weight_zero_is_the_step_without_the_argument():
    def run(lam):
        hs = _stepper(lam)
        x = _x().cuda()
        mets = []
        for s in range(2):
            hs.step(x, s, _eps(s).cuda())
            mets.append(hs.metrics())
        return _snapshot(hs), mets
    (a, ma), (b, mb) = run(None), run(0.0)
    for k in a:
        assert torch.equal(torch.as_tensor(a[k]), torch.as_tensor(b[k])), k
    assert ma == mb
    assert ma[-1]["reward_grad_loss"] == 0.0 and ma[-1]["eval_quality"] == 0.0


@pytest.mark.parametrize("full", [False, True], ids=["heads_only", "teacher_full_backward"])
def test_reward_pass_moves_nothing_of_the_teacher(full):
    """The teacher's flat state after its update, its gradients and its dropout stream are those of the lambda = 0 step: the eval pass
    writes none of them, and the teacher's own backward has read the train-mode call's tensors before the eval forward overwrote them."""
    def run(lam):
        hs = _stepper(lam, full=full)
        hs.step(_x().cuda(), 0, _eps().cuda())
        return _snapshot(hs)
    off, on, again = run(0.0), run(LAM), run(LAM)
    for k in ("t_flat", "t_grads", "nbt"):
        assert torch.equal(off[k], on[k]), k
    assert off["drop_calls"] == on["drop_calls"] > 0
    assert not torch.equal(off["grads"], on["grads"])                      # ... while the VAE's gradient does carry the term
    for k in on:
        assert torch.equal(torch.as_tensor(on[k]), torch.as_tensor(again[k])), k       # run to run


# ---- 5. accumulation ------------------------------------------------------------------------------------------------------------
def test_accumulation_runs_the_reward_pass_on_the_used_micro_batch_only():
    """accum = 2: the first micro-batch runs no reward pass; the second gives half the accum = 1 gradients.  Measured on the MI355X:
    4.5e-5 relative L2 (bound 1e-3)."""
    x, eps = _x().cuda(), _eps().cuda()
    hs = _stepper(LAM, accum=2, reward_scale=0.0, dropout=0.0)
    t = hs.teacher
    t._ensure_flat()
    flat, nbt = t._flat.clone(), t._nbt.clone()
    hs.step(x, 0, eps)
    torch.cuda.synchronize()
    assert hs._rg is None                                    # no seed buffer yet: the reward pass has not run
    # lo_teacher_last_path is still the train-mode forward's (0: the sparse path of the dropout-free teacher; the eval kept forward reports 1)
    assert t.last_path(B) == (1 if os.environ.get("LO_T_DENSE") == "1" else 0)
    assert hs.opt_steps == 0
    # the eval teacher reads the running statistics, which the first micro-batch's train-mode calls moved: put the state back, so that
    # the second micro-batch differentiates the function the accum = 1 step does (the accumulation and not the statistics is the subject)
    with torch.no_grad():
        t._flat.copy_(flat)
        t._nbt.copy_(nbt)
    hs.step(x, 1, eps)
    assert hs.opt_steps == 1 and hs._rg is not None and t.last_path(B) == 1
    half = _grads(hs)
    ref = [0.5 * g for g in _native("mixed")[0]]
    d = _global(half, ref)
    print(f"accum = 2 against half the accum = 1 gradients: {d:.4e}")
    assert d <= 1e-3, d


# ---- 6. lo_teacher_eval_backward_seed on guarded, poisoned memory ----------------------------------------------------------------
def _raw_seed(fill, coef, factor, seeded=True):
    """lo_teacher_forward_keep_eval + lo_teacher_eval_backward[_seed] on guard-banded buffers of exactly the header's sizes, ws / bws /
    rows pre-filled with the byte `fill`, dx with NaN; upstream rows of -2.  Returns dx."""
    from lunaris_orion_amd import _lib
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from tests.guarded import check_guards, gin, guarded, written
    lib, st = _lib.lib, _lib.stream_ptr()
    n = 3
    t = LunarMoETeacher()
    t.load_state_dict(T.closed_form_teacher_state())
    t = t.to("cuda").eval()
    t._ensure_flat()
    h = C.c_void_p()
    _lib.check(lib.lo_teacher_create_ex(n, 4, 128, 64, 0, C.byref(h)), "create")
    try:
        flat = gin(t._flat)
        x = gin(_x(n))
        target = gin(_x(n).flip(0))
        ws = guarded(lib.lo_teacher_workspace_bytes(h), torch.uint8, "ws", payload_fill=fill)
        bws = guarded(lib.lo_teacher_full_backward_bytes(h), torch.uint8, "ws", payload_fill=fill)
        _lib.check(lib.lo_teacher_pack(h, flat.data_ptr(), ws.data_ptr(), st), "pack")
        outs = [guarded(s, torch.float32, "out") for s in ((n, 4), (n, 4), (n, 64), (n, 64), (n, 1))]
        _lib.check(lib.lo_teacher_forward_keep_eval(h, x.data_ptr(), flat.data_ptr(), ws.data_ptr(), bws.data_ptr(), *[o.data_ptr() for o in outs], st),
                   "lo_teacher_forward_keep_eval")
        offs, elems = (C.c_size_t * 3)(), (C.c_size_t * 3)()
        _lib.check(lib.lo_teacher_heads_saved(h, offs, elems), "saved")
        saved = [gin(ws[offs[i]:offs[i] + 4 * elems[i]].view(torch.float32).clone()) for i in range(3)]
        weights = gin(outs[1].clone())
        b, e = C.c_size_t(), C.c_size_t()
        _lib.check(lib.lo_teacher_grad_range(h, C.byref(b), C.byref(e)), "range")
        rows = guarded(n * (e.value - b.value), torch.float32, "ws", payload_fill=fill)
        dq = gin(torch.full((n, 4), -2.0))
        cdev = gin(torch.full((1,), float(coef)))
        dx = guarded((n, 3, 128, 128), torch.float32, "out")
        head = (h, x.data_ptr(), flat.data_ptr(), ws.data_ptr(), bws.data_ptr(), *[s.data_ptr() for s in saved], weights.data_ptr(), dq.data_ptr(),
                None, float(2 ** 20), rows.data_ptr())
        if seeded:
            _lib.check(lib.lo_teacher_eval_backward_seed(*head, target.data_ptr(), cdev.data_ptr(), float(factor), dx.data_ptr(), st),
                       "lo_teacher_eval_backward_seed")
        else:
            _lib.check(lib.lo_teacher_eval_backward(*head, None, dx.data_ptr(), st), "lo_teacher_eval_backward")
        torch.cuda.synchronize()
        check_guards(flat, x, target, ws, bws, rows, dq, weights, cdev, dx, *outs, *saved)
        written(dx, *outs)
        assert torch.equal(flat, t._flat)                        # flat_state is const: not one byte
        return dx.cpu(), x.cpu(), target.cpu()
    finally:
        lib.lo_teacher_destroy(h)


def test_eval_backward_seed_raw_abi_on_guarded_poisoned_memory():
    plain = _raw_seed(0xFF, 0.0, 1.0, seeded=False)[0]
    zero_ff, zero_00 = _raw_seed(0xFF, 0.0, 1.0)[0], _raw_seed(0x00, 0.0, 1.0)[0]
    assert torch.equal(zero_ff, plain) and torch.equal(zero_00, plain)         # scalar 0, factor 1: the bits of lo_teacher_eval_backward
    c, f = 0.125, 0.25                                                          # powers of two: scaling the fp32 result is exact
    got, x, target = _raw_seed(0xFF, c, f)
    ref = f * plain.double() + c * (x.double() - target.double())
    print("seeded eval backward against factor * dx + c * (x - target):", _rel(got, ref))
    assert _rel(got, ref) <= 1e-6, _rel(got, ref)
