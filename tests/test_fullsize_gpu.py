"""Parity at BASELINE.json's full sizes (batch 64, latent 512) through size-independent properties.

The oracle needs minutes per step at this size, so the full-size runs are tied to it indirectly:
  * GroupNorm is per-sample and the losses are means, so sample i of a batch-64 forward must equal the same sample in a
    batch-2 forward (which tests/test_vae_gpu.py checks against the oracle and the golden fixtures);
  * the losses must equal the plain means over the returned tensors;
  * the batch-64 gradient must be the average of the gradients of its two batch-32 halves;
  * the same step twice gives the same bits;
  * the teacher in eval mode (running statistics) is per-sample too: batch 64 vs batch 2; in train mode the sparse
    expert path must reproduce the dense path (every convolution in full) at batch 64.
The direct tie at batch 64 is tests/test_vae_insitu_gpu.py: every layer of one batch-64 step against an fp64 reference of its own operands.
Tolerances: mu / logvar / recon 5e-3 abs (different tile shapes are picked at different batch sizes, so
the fp32 accumulation order differs), losses 1e-4 abs, gradients 2e-3 relative L2 (fp16 activations).
"""
import os
import subprocess
import sys

import pytest
import torch

from oracle import teacher_ref as T
from oracle import vae_ref as R

pytestmark = pytest.mark.gpu
B_FULL, L_FULL = 64, 512
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _vae(L=L_FULL):
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(latent_dim=L)
    m.load_state_dict(R.closed_form_params(L, 0))
    return m.to("cuda")


def _inputs(B, L=L_FULL):
    x = R.normalise_sprites(R.closed_form_sprites(B)).cuda()
    eps = R.closed_form_eps(B, L, salt=0).cuda()
    return x, eps


def test_batch64_forward_is_per_sample_and_losses_are_means():
    m = _vae()
    x, eps = _inputs(B_FULL)
    with torch.no_grad():
        recon, mu, logvar = m(x, eps)
        # the pair (4, 37) as its own batch of two
        idx = torch.tensor([4, 37], device="cuda")
        r2, mu2, lv2 = m(x[idx].contiguous(), eps[idx].contiguous())
    torch.cuda.synchronize()
    assert (mu[idx] - mu2).abs().max().item() <= 5e-3
    assert (logvar[idx] - lv2).abs().max().item() <= 5e-3
    assert (recon[idx] - r2).abs().max().item() <= 5e-3
    # tie the small batch to the oracle here as well (seconds on the CPU)
    P = R.closed_form_params(L_FULL, 0)
    r_ref, mu_ref, lv_ref = R.vae_forward(x[idx].cpu(), eps[idx].cpu(), P)
    assert (mu2.cpu() - mu_ref).abs().max().item() <= 5e-3
    assert (lv2.cpu() - lv_ref).abs().max().item() <= 5e-3
    assert (r2.cpu() - r_ref).abs().max().item() <= 5e-3

    from lunaris_orion_amd.trainer import VAEStepper
    st = VAEStepper(m, lr=0.0, weight_decay=0.0)
    st.step(x, 0, eps)
    met = st.metrics()
    rl = torch.mean((recon.double() - x.double()) ** 2).item()
    kl = (-0.5 * torch.mean(1 + logvar.double() - mu.double() ** 2 - logvar.double().exp())).item()
    assert abs(met["recon_loss"] - rl) <= 1e-4
    assert abs(met["kl_loss"] - kl) <= 1e-4


def test_batch64_gradient_is_the_mean_of_its_halves_and_is_deterministic():
    from lunaris_orion_amd.trainer import VAEStepper
    x, eps = _inputs(B_FULL)

    def grads(xs, es):
        m = _vae()
        st = VAEStepper(m, lr=0.0, weight_decay=0.0, max_grad_norm=1e9)
        st.step(xs, 0, es)
        torch.cuda.synchronize()
        return [g.detach().double().clone() for g in st.parameter_grads()], [k for k, _ in m.named_parameters()]

    full, names = grads(x, eps)
    again, _ = grads(x, eps)
    for a, b, k in zip(full, again, names):
        assert torch.equal(a, b), k                       # bitwise run-to-run
    h0, _ = grads(x[:32].contiguous(), eps[:32].contiguous())
    h1, _ = grads(x[32:].contiguous(), eps[32:].contiguous())
    num = den = 0.0
    for g, a, b, k in zip(full, h0, h1, names):
        ref = 0.5 * (a + b)
        e, n = (g - ref).norm().item(), ref.norm().item()
        num += e * e
        den += n * n
        assert e <= 2e-3 * n + 1e-9, (k, e / (n + 1e-30))
    assert (num / den) ** 0.5 <= 1e-3


def test_full_size_clip_adamw_matches_torch():
    """clip_grad_norm_ + AdamW on the whole latent-512 flat buffer (61 M elements) against torch.optim.AdamW."""
    from lunaris_orion_amd.trainer import VAEStepper
    m = _vae()
    x, eps = _inputs(4)
    st = VAEStepper(m, lr=1e-3, min_lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
    before = [p.detach().clone() for p in m.parameters()]
    st.step(x, 0, eps)
    torch.cuda.synchronize()
    g = [t.detach().clone() for t in st.parameter_grads()]
    ref = [torch.nn.Parameter(b.clone()) for b in before]
    for p, gg in zip(ref, g):
        p.grad = gg.clone()
    opt = torch.optim.AdamW(ref, lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
    torch.nn.utils.clip_grad_norm_(ref, 1.0)
    opt.step()
    for (k, p), r in zip(m.named_parameters(), ref):
        assert (p.detach() - r.detach()).abs().max().item() <= 2e-6, k


def _teacher(B):
    from lunaris_orion_amd.teacher import LunarMoETeacher
    m = LunarMoETeacher(num_experts=4, feature_dim=128, embedding_dim=256, dropout_rate=0.0)
    m.load_state_dict(T.closed_form_teacher_state(embedding_dim=256))
    return m.to("cuda")


def test_teacher_eval_batch64_is_per_sample():
    m = _teacher(B_FULL)
    m.eval()
    x, _ = _inputs(B_FULL)
    idx = torch.tensor([9, 50], device="cuda")
    with torch.no_grad():
        full = m(x)
        two = m(x[idx].contiguous())
    torch.cuda.synchronize()
    tol = {"quality_scores": 2e-3, "expert_weights": 2e-3, "style_embedding": 2e-2, "prompt_embedding": 2e-2, "semantic_score": 2e-3}
    for k, t in tol.items():
        assert (full[k][idx] - two[k]).abs().max().item() <= t, k


_DENSE_SNIPPET = r"""
import sys, torch
sys.path.insert(0, {root!r})
from oracle import vae_ref as R
from lunaris_orion_amd.teacher import LunarMoETeacher
from oracle import teacher_ref as T
m = LunarMoETeacher(num_experts=4, feature_dim=128, embedding_dim=256, dropout_rate=0.0)
m.load_state_dict(T.closed_form_teacher_state(embedding_dim=256))
m = m.to("cuda")
m.train(True)
x = R.normalise_sprites(R.closed_form_sprites(64)).cuda()
out = m(x)
torch.cuda.synchronize()
torch.save({{k: v.cpu() for k, v in out.items() if v is not None}} | {{"rm": m.state_dict()["experts.3.2.conv2.2.running_mean"].cpu(),
            "rv": m.state_dict()["experts.1.1.conv1.2.running_var"].cpu()}}, sys.argv[1])
"""


def test_teacher_train_batch64_sparse_equals_dense(tmp_path):
    """The path that skips the constant fields (default) against every convolution in full (LO_T_DENSE=1), batch 64,
    train-mode BatchNorm: outputs and the running statistics it leaves behind.  One process each: the switch is read
    when the library creates the teacher."""
    outs = {}
    for dense in ("0", "1"):
        f = tmp_path / f"t{dense}.pt"
        env = dict(os.environ, LO_T_DENSE=dense)
        r = subprocess.run([sys.executable, "-c", _DENSE_SNIPPET.format(root=ROOT), str(f)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[dense] = torch.load(f)
    tol = {"quality_scores": 2e-3, "expert_weights": 2e-3, "style_embedding": 2e-2, "prompt_embedding": 2e-2, "semantic_score": 2e-3,
           "rm": 2e-3, "rv": 2e-3}
    for k, t in tol.items():
        d = (outs["0"][k] - outs["1"][k]).abs().max().item()
        assert d <= t * max(1.0, outs["1"][k].abs().max().item()), (k, d)


def test_teacher_train_batch64_default_dropout_matches_the_oracle():
    """The configuration BASELINE config 3 TIMES, checked directly: batch 64, train mode, the reference's default
    dropout 0.1, default kernel selection -- every 3x3 convolution in full on the fused-tap kernel (`last_path == 2`), the
    long-grid tile choices of the U / proj / pointwise GEMMs -- against the oracle's functions on the same masks (all 64 samples:
    train-mode BatchNorm couples them; evaluated on device tensors, tests/hip_helpers.py: the CPU evaluation took 82 s of the suite),
    outputs and the running statistics the call leaves behind."""
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from oracle import dropout_ref as D
    B, seed, p = B_FULL, 0x64640BADC0FFEE01, 0.1
    S = T.closed_form_teacher_state(embedding_dim=256)
    m = LunarMoETeacher(num_experts=4, feature_dim=128, embedding_dim=256)            # dropout_rate 0.1, like train_hybrid.py:400-404
    m.load_state_dict(S)
    m = m.to("cuda").train()
    m.set_dropout_stream(seed, exact_next=True)
    x = R.normalise_sprites(R.closed_form_sprites(B))
    with torch.no_grad():
        out = m(x.cuda())
    torch.cuda.synchronize()
    assert m.last_path(B) == 2 and m.last_drop_seed == seed
    from tests.hip_helpers import oracle_teacher_on_device
    ref, new_stats = oracle_teacher_on_device(x, S, True, seed, p)
    tol = {"quality_scores": 2e-3, "expert_weights": 2e-3, "style_embedding": 2e-2, "prompt_embedding": 2e-2, "semantic_score": 2e-3}
    for k, t in tol.items():
        d = (out[k].cpu() - ref[k]).abs().max().item()
        print("B=64 dropout", k, d)
        assert d <= t, (k, d)
    sd = m.state_dict()
    for k in ("experts.3.2.conv2.2.running_mean", "experts.1.1.conv1.2.running_var", "feature_extractor.fusion.2.running_var"):
        r = new_stats[k]
        assert (sd[k].cpu() - r).abs().max().item() <= 2e-3 * max(1.0, r.abs().max().item()), k


def test_config2_shape_batch32_latent256():
    """BASELINE config 2's exact shape (batch 32, latent 256, VAE-only): samples of the batch-32 forward equal the same samples
    run as a batch of 2 (which test_vae_gpu checks against the oracle and the reference fixture), the losses are the means of
    the returned tensors, the step is bitwise reproducible, and the batch-32 gradient is the mean of its batch-16 halves."""
    from lunaris_orion_amd.trainer import VAEStepper
    B, L = 32, 256
    x, eps = _inputs(B, L)
    m = _vae(L)
    with torch.no_grad():
        recon, mu, logvar = m(x, eps)
        r2, mu2, lv2 = m(x[30:32].contiguous(), eps[30:32].contiguous())
    torch.cuda.synchronize()
    assert (mu[30:32] - mu2).abs().max().item() <= 5e-3 and (logvar[30:32] - lv2).abs().max().item() <= 5e-3
    assert (recon[30:32] - r2).abs().max().item() <= 5e-3

    def grads(xs, es):
        mm = _vae(L)
        st = VAEStepper(mm, lr=0.0, weight_decay=0.0, max_grad_norm=1e9)
        st.step(xs, 0, es)
        met = st.metrics()
        return [g.detach().double().clone() for g in st.parameter_grads()], met, [k for k, _ in mm.named_parameters()]
    full, met, names = grads(x, eps)
    again, _, _ = grads(x, eps)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    rl = torch.mean((recon.double() - x.double()) ** 2).item()
    kl = (-0.5 * torch.mean(1 + logvar.double() - mu.double() ** 2 - logvar.double().exp())).item()
    assert abs(met["recon_loss"] - rl) <= 1e-4 and abs(met["kl_loss"] - kl) <= 1e-4
    h0, _, _ = grads(x[:16].contiguous(), eps[:16].contiguous())
    h1, _, _ = grads(x[16:].contiguous(), eps[16:].contiguous())
    for g, a, b, k in zip(full, h0, h1, names):
        ref = 0.5 * (a + b)
        assert (g - ref).norm().item() <= 2e-3 * ref.norm().item() + 1e-9, k


def test_hybrid_step_batch64_latent512_composition_against_the_oracle():
    """BASELINE config 3 as `bench.py` times it (batch 64, latent 512, embedding 256, teacher with the reference's default dropout),
    checked as a COMPOSITION (the full hybrid step at this size only ran under a finite-loss assertion):
      * the VAE half of the step is the VAE-only step bit for bit (same weights, same noise): recon / KL losses, reconstruction;
      * the teacher call that is evaluated (train_hybrid.py:865, `teacher(recon.detach())`) against the oracle's functions on the
        same input and the same dropout masks (the call's seed is read back from the module), all 64 samples;
      * reward / baseline / advantage / losses follow train_hybrid.py:867-892 from those outputs, first step (baseline = batch mean,
        advantage exactly 0) and second step (EMA baseline with momentum 0.9, advantage scaled by reward_scale 0.1);
      * the second step is finite, nothing was skipped, and only the gate / quality heads of the teacher moved."""
    from lunaris_orion_amd.teacher import LunarMoETeacher
    from lunaris_orion_amd.trainer import HybridStepper, VAEStepper
    from tests.hip_helpers import oracle_teacher_on_device
    B, L = B_FULL, L_FULL
    x, eps = _inputs(B)
    S = T.closed_form_teacher_state(embedding_dim=256)
    vae = _vae()
    t = LunarMoETeacher(num_experts=4, feature_dim=128, embedding_dim=256)
    t.load_state_dict(S)
    t = t.to("cuda").train()
    t.set_dropout_stream(0xC0FFEE64, exact_next=True)
    conv_before = t.experts[2][1].conv2[0].weight.detach().clone()
    gate_before = t.gate[2].weight.detach().clone()
    hs = HybridStepper(vae, t, gradient_accumulation_steps=1, pipeline_optimizer=True)
    recon, mu, logvar = hs.step(x, 0, eps)
    m0 = hs.metrics()
    seed_eval = t.last_drop_seed                      # the evaluated call is the step's second teacher call
    out = {k: v.detach().cpu() for k, v in hs.last_teacher_out.items() if torch.is_tensor(v)}
    assert t.last_path(B) == 2
    # ---- VAE half == the VAE-only step
    vs = VAEStepper(_vae(), gradient_accumulation_steps=1, pipeline_optimizer=True)
    r2, _, _ = vs.step(x, 0, eps)
    v0 = vs.metrics()
    assert m0["recon_loss"] == v0["recon_loss"] and m0["kl_loss"] == v0["kl_loss"] and torch.equal(recon, r2)
    # ---- the evaluated teacher call against the oracle's functions (BatchNorm statistics as the first, statistics-only call left them)
    t_ref = LunarMoETeacher(num_experts=4, feature_dim=128, embedding_dim=256)
    t_ref.load_state_dict(S)
    t_ref = t_ref.to("cuda").train()
    t_ref.set_dropout_stream(0xC0FFEE64, exact_next=True)
    t_ref.update_statistics_only(x)                   # train_hybrid.py:853-855: running statistics move, batch statistics are used
    S1 = {k: v.detach().cpu() for k, v in t_ref.state_dict().items()}
    ref, _ = oracle_teacher_on_device(recon.detach().cpu(), S1, True, seed_eval, 0.1)
    for k, tol in (("quality_scores", 2e-3), ("semantic_score", 2e-3), ("expert_weights", 2e-3)):
        d = (out[k] - ref[k]).abs().max().item()
        print("hybrid B=64 teacher", k, d)
        assert d <= tol, (k, d)
    # ---- reward bookkeeping, first step
    q, sem = out["quality_scores"].double(), out["semantic_score"].double()
    quality_reward = q.mean(dim=1, keepdim=True)
    total = quality_reward + 0.5 * sem
    base0 = total.mean().item()
    assert abs(m0["quality_reward"] - quality_reward.mean().item()) <= 1e-5 and abs(m0["semantic_reward"] - sem.mean().item()) <= 1e-5
    assert abs(m0["baseline"] - base0) <= 1e-5 and m0["advantage"] == 0.0 and m0["pg_loss"] == 0.0
    assert abs(m0["quality_loss"] + q.mean().item()) <= 1e-5 and abs(m0["teacher_loss"] - 0.5 * m0["quality_loss"]) <= 1e-6
    assert abs(m0["vae_loss"] - (m0["recon_loss"] + 0.1 * m0["kl_loss"])) <= 1e-6
    # ---- second step
    hs.step(x, 1, R.closed_form_eps(B, L, salt=1).cuda())
    m1 = hs.metrics()
    o1 = {k: v.detach().cpu().double() for k, v in hs.last_teacher_out.items() if torch.is_tensor(v)}
    tr1 = (o1["quality_scores"].mean(dim=1, keepdim=True) + 0.5 * o1["semantic_score"]).mean().item()
    base1 = 0.9 * base0 + 0.1 * tr1
    adv1 = (tr1 - base1) * 0.1
    assert abs(m1["baseline"] - base1) <= 1e-5 and abs(m1["advantage"] - adv1) <= 1e-6
    assert abs(m1["pg_loss"] + adv1 * m1["recon_loss"]) <= 1e-6
    assert abs(m1["vae_loss"] - (m1["recon_loss"] + 0.1 * m1["kl_loss"] + m1["pg_loss"])) <= 1e-6
    assert all(torch.isfinite(torch.tensor(float(v))) for v in m1.values()) and m1["grads_finite"] == 1.0 and m1["skipped_steps"] == 0.0
    hs.synchronize_parameters()
    torch.cuda.synchronize()
    assert not torch.equal(t.gate[2].weight, gate_before) and torch.equal(t.experts[2][1].conv2[0].weight, conv_before)
