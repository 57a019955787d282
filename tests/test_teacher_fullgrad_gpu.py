"""SURVEY §8 row F2, second half: `lo_teacher_full_backward` -- gradients for every teacher parameter on the path of the teacher
loss, experts and feature extractor included (lunar_evaluator.py:194-197, 266-275, 411-414 with non-reentrant checkpoints;
train_hybrid.py:891-904).  Checked against
  * the reference itself: tests/golden/teacher_fullgrad_{,drop_}B2.npz (oracle/make_golden.py run_teacher_fullgrad: the reference's
    modules, `checkpoint` made non-reentrant in-process, its own dropout modules on injected masks) -- sums, norms and 2048 sampled
    entries of all 234 gradients;
  * autograd of the CPU oracle (oracle/teacher_ref.py) on the same inputs, every tensor in full.
Tolerance against the fp32 oracle and the fixture: 4e-2 of the tensor's norm, and cosine >= 0.999 with the norm within 1 % for every
tensor that carries a visible share of the total.  What that tolerance covers was measured (tools/README.md): the deviation
is unbiased noise (cosine 0.9997-1.0000, norm ratio 1 +- 0.005; independent of the gradient scale 2^17 ... 2^25), 0.1-0.7 % in the
feature extractor, BatchNorm and layer-scale gradients and 1-2.9 % in the conv / attention weights of the expert blocks.  Tensors whose
gradient is mathematically zero are compared on an absolute scale.

Where that noise comes from was tested, not assumed (the tests at the end of this module, tests/test_teacher_oracle_rounded.py):
the oracle with ``act_dtype=torch.float16`` rounds to fp16 exactly where the plain-form forward does (straight-through gradient, LeakyReLU
slope from the stored value).  Measured on the MI355X, worst d / max(|o|, 1e-3 total) per group, feature_dim 128, batch 2, over the four
(dropout, kept forward) cases -- against the rounding oracle | against the fp32 oracle:
    feature extractor                         1.1e-3 | 7.4e-3      -> bound 3e-3
    BatchNorm weight / bias, layer_scale      5.8e-3 | 7.0e-3      -> bound 2e-2
    heads / gate (plain-form forward)         5.6e-5 | 6.8e-3      -> bound 2e-4
    heads / gate (folded production forward)  6.8e-3 | 1.1e-3      -> bound 2e-2  (no dropout, not kept: the heads then read the pooled
                                                                      features of the folded feature_dim-128 path, another rounding pattern)
    block conv / qkv / proj weights + biases  1.8e-2 | 2.9e-2      -> bound 4e-2: NOT tighter than before, see below
    input-image gradient (test_input_grad_gpu) 1.3e-2 | 6.4e-2, 16x16-pooled 1.9e-3 | 8.4e-3   -> bounds 3e-2, 4e-3
    feature_dim 256, batch 1, dropout 0.1:    fe 2.6e-3 | 8.2e-3, BatchNorm / layer_scale 5.9e-3 | 9.7e-3, heads 4.6e-5 | 6.3e-4,
                                              block conv / qkv / proj 3.3e-2 | 4.4e-2    -> bounds 6e-3, 2e-2, 1e-4, 7e-2 (not tighter)
    BatchNorm running statistics, 29 layers   batch mean 4.0e-4 of a standard deviation (one layer; all others <= 2e-5) | 2.3e-3, batch variance
                                              1.6e-5 | 8.8e-4 relative   -> bounds 8e-4, 4e-5; head outputs 1.3e-6 ... 1.7e-5 | 6.6e-5 ... 2.8e-4
Each bound is twice the measured worst, rounded up to one digit.  "LeakyReLU's kink under fp16 activations" is confirmed for the feature
extractor, the heads and the input gradient (5-7x closer to the rounding oracle; the forward itself agrees to 1e-5 of a standard deviation
in every BatchNorm layer's batch mean).  For the expert blocks' conv / qkv / proj gradients it explains a third; the remaining 1.2 % (no
dropout) to 1.8 % (dropout 0.1) is no missed rounding site: perturbing the ORACLE by one part in 1e7 in front of its roundings -- another
fp32 summation order -- moves exactly these tensors by 0.6 % (median) to 2.6 % and the other groups by what they show here
(tests/test_teacher_oracle_rounded.py).  conv2's output is close to a constant field whose batch standard deviation is a few fp16 ulp, so an
element that rounds the other way moves BatchNorm2's normalised tensor by a visible fraction of 1.  An oracle cannot take that group below
about 2 % at batch 2; a mis-scaled term of 3 % there is caught through the same block's BatchNorm / layer_scale gradients (2e-2).
"""
import os

import numpy as np
import pytest
import torch

from oracle import dropout_ref as D
from oracle import teacher_ref as T
from oracle import vae_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
DROP_SEED, DROP_P, QW = 0x5EEDD209C0FFEE11, 0.1, 0.5


def _teacher(drop, F=128, emb=64):
    from lunaris_orion_amd.teacher import LunarMoETeacher
    kw = {} if F == 128 else {"feature_dim": F, "embedding_dim": emb}
    m = LunarMoETeacher(num_experts=4, feature_dim=F, embedding_dim=emb, dropout_rate=DROP_P if drop else 0.0)
    m.load_state_dict(T.closed_form_teacher_state(**kw))
    m = m.to("cuda")
    m.train()
    return m


_ORACLE_CACHE = {}


def _oracle_run(x, drop, device="cpu", act_dtype=None, **kw):
    key = (tuple(x.shape), bool(drop), device, act_dtype, tuple(sorted(kw.items())))
    if key not in _ORACLE_CACHE:              # inputs are closed-form: the same (shape, dropout) always means the same numbers
        extras = {}
        _ORACLE_CACHE[key] = _oracle_grads_uncached(x, drop, device, act_dtype=act_dtype, extras=extras, **kw) + (extras,)
    return _ORACLE_CACHE[key]


def _oracle_grads(x, drop, device="cpu", **kw):
    return _oracle_run(x, drop, device, **kw)[:2]


def _oracle_extras(x, drop, device="cpu", act_dtype=None, **kw):
    """{"x_grad", "new_stats", "out"} of the cached oracle run (act_dtype=torch.float16: the fp16-rounding oracle)."""
    return _oracle_run(x, drop, device, act_dtype, **kw)[2]


def _oracle_grads_uncached(x, drop, device="cpu", act_dtype=None, extras=None, **kw):
    S = T.closed_form_teacher_state(**kw)
    P = {k: (v.to(device).clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and "last_spatial" not in k else v.to(device))
         for k, v in S.items()}
    masks = D.TeacherMasks(DROP_SEED, DROP_P, x.shape[0], device=device) if drop else None
    xd = x.to(device)
    if extras is not None:
        xd = xd.clone().requires_grad_(True)
    out, stats = T.teacher_forward(xd, P, training=True, masks=masks, act_dtype=act_dtype)
    loss = QW * -torch.mean(out["quality_scores"])
    names = [k for k, v in P.items() if v.requires_grad]
    g = torch.autograd.grad(loss, [P[k] for k in names] + ([xd] if extras is not None else []), allow_unused=True)
    if extras is not None:
        extras.update(x_grad=g[-1].detach().cpu(), new_stats={k: v.detach().cpu() for k, v in stats.items()},
                      out={k: v.detach().cpu() for k, v in out.items()})
    return {k: (None if t is None else t.detach().cpu()) for k, t in zip(names, g)}, loss.item()


def _native_grads(m, x, drop, keep=False):
    if drop:
        m.set_dropout_stream(DROP_SEED, exact_next=True)
    with torch.no_grad():
        out = m._native_forward(x, keep=True)[0] if keep else m(x)       # keep: lo_teacher_forward_keep, no first pass in the backward
    flat = m.full_backward(x, out["expert_weights"], QW)
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in m.parameter_grad_views(flat).items()}, out


def _zero_by_construction(k):
    # a conv bias in front of a train-mode BatchNorm shifts the batch mean and nothing else -- but only where no LeakyReLU sits
    # between them: in this model every such conv is followed by LeakyReLU, except the shortcut conv (feature_dim != 128)
    return k.endswith("shortcut.0.bias")


@pytest.mark.parametrize("drop,keep", [(False, False), (True, False), (True, True)], ids=["no_dropout", "dropout_0.1", "dropout_0.1_kept_forward"])
def test_full_backward_matches_the_reference_fixture_and_the_oracle(drop, keep):
    """keep: the step's forward is lo_teacher_forward_keep (plain expert path, block outputs left in the backward's scratch: what
    HybridStepper(teacher_full_backward=True) runs); otherwise the production forward, and the backward recomputes them itself."""
    B = 2
    x = R.normalise_sprites(R.closed_form_sprites(B))
    m = _teacher(drop)
    got, out = _native_grads(m, x.cuda(), drop, keep)
    if keep:
        # the kept forward is the same function as the production one: outputs against the oracle's at the forward tolerances
        oo, _ = T.teacher_forward(x, T.closed_form_teacher_state(), training=True, masks=D.TeacherMasks(DROP_SEED, DROP_P, B))
        assert (out["quality_scores"].cpu() - oo["quality_scores"]).abs().max().item() <= 2e-3
        assert (out["style_embedding"].cpu() - oo["style_embedding"]).abs().max().item() <= 2e-2
    ora, _ = _oracle_grads(x, drop)
    z = np.load(os.path.join(GOLD, f"teacher_fullgrad_{'drop_' if drop else ''}B2.npz"))
    assert int(z["n_with_grad"]) == 234
    worst = {}
    n_checked = 0
    for k, g in got.items():
        o = ora.get(k)
        if o is None:
            # off the loss path (style / prompt / semantic heads) or the softmax-invariant relative-position tables: exactly zero here
            assert g.abs().max().item() == 0.0, k
            continue
        n_checked += 1
        on, d = o.norm().item(), (g - o).norm().item()
        scale = max(on, 1e-3 * float(z["total_norm"]))
        worst[k] = d / scale
        assert d <= 4e-2 * scale, (k, d, on)
        if on >= 1e-3 * float(z["total_norm"]):
            cos = torch.nn.functional.cosine_similarity(g.flatten().double(), o.flatten().double(), dim=0).item()
            assert cos >= 0.999 and abs(g.norm().item() / on - 1.0) <= 1e-2, (k, cos, g.norm().item() / on)
        # the reference's own numbers (sampled entries)
        tag = f"tgrad/{k}"
        idx = ((R.closed_form_uniform("sample." + tag, min(2048, g.numel())) + 1.0) * 0.5 * g.numel()).long().clamp_(0, g.numel() - 1)
        ref = torch.from_numpy(z[tag + "/samples"])
        ds = (g.flatten()[idx] - ref).norm().item()
        assert ds <= 4e-2 * max(ref.norm().item(), 1e-3 * float(z["total_norm"]) * (len(idx) / g.numel()) ** 0.5) + 1e-12, (k, ds, ref.norm().item())
    assert n_checked == 234 - 24          # 24 relative-position tables are off the oracle's graph
    tot = torch.sqrt(sum((g.double() ** 2).sum() for g in got.values())).item()
    assert abs(tot - float(z["total_norm"])) <= 1e-2 * float(z["total_norm"]), (tot, float(z["total_norm"]))
    print("worst relative errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:8])


@pytest.mark.parametrize("F", [256, 512])
def test_full_backward_wide_teacher_shortcut_branch_matches_the_oracle(F):
    """feature_dim != 128 (512 = the README High-End recipe): the first block of every expert has the Conv1x1 + BatchNorm shortcut
    (lunar_evaluator.py:254-257), 32- / 64-wide heads; the oracle's autograd runs on the device (same functions, ATen fp32 kernels)."""
    B, emb = 1, 256
    x = R.normalise_sprites(R.closed_form_sprites(B))
    m = _teacher(True, F, emb)
    got, _ = _native_grads(m, x.cuda(), True)
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        ora, _ = _oracle_grads(x, True, device="cuda", feature_dim=F, embedding_dim=emb)
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
    tot = torch.sqrt(sum((o.double() ** 2).sum() for o in ora.values() if o is not None)).item()
    n = 0
    for k, g in got.items():
        o = ora.get(k)
        if o is None:
            assert g.abs().max().item() == 0.0, k
            continue
        n += 1
        d, on = (g - o).norm().item(), o.norm().item()
        if _zero_by_construction(k):
            assert on <= 1e-4 * tot and g.norm().item() <= 2e-3 * tot, (k, on, g.norm().item())
            continue
        # one sample instead of two and twice the channels: the kink noise of the module docstring is 1.5x larger here (measured
        # worst 4.3 %); a missing or mis-scaled term would show in the cosine / the norm ratio, which stay tight
        assert d <= 6e-2 * max(on, 1e-3 * tot), (k, d, on)
        if on >= 1e-3 * tot:
            cos = torch.nn.functional.cosine_similarity(g.flatten().double(), o.flatten().double(), dim=0).item()
            assert cos >= 0.998 and abs(g.norm().item() / on - 1.0) <= 1e-2, (k, cos, g.norm().item() / on)
    assert n == 234 + 4 * 4 - 24          # + shortcut conv weight / bias and BatchNorm weight / bias per expert


def test_full_parameter_update_touches_exactly_what_the_reference_optimizer_would():
    """lo_teacher_clip_adamw_full against torch.optim.AdamW fed with the SAME gradients (clip_grad_norm_ first), two steps: every tensor
    with a gradient moves as AdamW says (the relative-position tables by weight decay alone), BatchNorm buffers and the three heads
    the loss does not read stay bit-identical, and the forward after the update sees the new weights (operand re-pack)."""
    import ctypes as C
    from lunaris_orion_amd import _lib
    B, lr, wd, max_norm = 2, 1e-3, 0.01, 0.05
    x = R.normalise_sprites(R.closed_form_sprites(B)).cuda()
    m = _teacher(True)
    names = [k for k, _ in m.named_parameters()]
    off_path = lambda k: k.split(".")[0] in ("semantic_head", "style_net", "prompt_net")
    ref_p = {k: p.detach().clone().requires_grad_(True) for k, p in m.named_parameters() if not off_path(k)}
    opt = torch.optim.AdamW(list(ref_p.values()), lr=lr, weight_decay=wd, betas=(0.9, 0.999), eps=1e-8)
    eng = m._engine(B)
    nt, ne = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.lib.lo_teacher_full_param_count(eng.handle, C.byref(nt), C.byref(ne)), "count")
    assert nt.value == len(ref_p) == 234 and ne.value == sum(p.numel() for p in ref_p.values())
    mm, vv = torch.zeros_like(m._flat), torch.zeros_like(m._flat)
    scratch = torch.zeros(1028, device="cuda")
    state0 = {k: v.detach().clone() for k, v in m.state_dict().items()}
    q_before = None
    for step in (1, 2):
        m.set_dropout_stream(DROP_SEED + step, exact_next=True)
        with torch.no_grad():
            out = m(x)
        if q_before is None:
            q_before = out["quality_scores"].clone()
        stats = {k: v.detach().clone() for k, v in m.state_dict().items() if "running" in k}
        flat = m.full_backward(x, out["expert_weights"], QW)
        gv = m.parameter_grad_views(flat)
        for k, p in ref_p.items():
            p.grad = gv[k].detach().clone()
        torch.nn.utils.clip_grad_norm_(list(ref_p.values()), max_norm)
        opt.step()
        _lib.check(_lib.lib.lo_teacher_clip_adamw_full(eng.handle, m._flat.data_ptr(), flat.data_ptr(), mm.data_ptr(), vv.data_ptr(), max_norm, lr,
                                                       0.9, 0.999, 1e-8, wd, step, scratch.data_ptr(), _lib.stream_ptr()), "clip_adamw_full")
        m.mark_weights_changed()
        torch.cuda.synchronize()
        for k, v in m.state_dict().items():
            if "running" in k:
                assert torch.equal(v, stats[k]), k                                   # buffers are not parameters
    sd = m.state_dict()
    for k in names:
        if off_path(k):
            assert torch.equal(sd[k], state0[k]), k
            continue
        a, b = sd[k], ref_p[k].detach()
        assert (a - b).abs().max().item() <= 2e-6 + 1e-5 * b.abs().max().item(), (k, (a - b).abs().max().item())
        assert not torch.equal(a, state0[k]), k                                       # every live tensor moved
    with torch.no_grad():
        m.set_dropout_stream(DROP_SEED + 1, exact_next=True)
        q_after = m(x)["quality_scores"]
    assert torch.isfinite(q_after).all() and not torch.equal(q_after, q_before)
    assert q_after.mean().item() > q_before.mean().item()                             # the loss is -mean(quality_scores): two steps up


def test_hybrid_stepper_with_teacher_full_backward_runs_the_whole_step():
    """`--teacher_full_backward` end to end: HybridStepper(teacher_full_backward=True), three steps of the full hybrid _process_batch;
    the expert and feature-extractor weights move, the metrics stay finite, and the default (flag off) leaves them alone."""
    from lunaris_orion_amd.trainer import HybridStepper
    from lunaris_orion_amd.vae import LunarisCoreVAE
    B, L = 2, 256
    x = R.normalise_sprites(R.closed_form_sprites(B)).cuda()
    moved = {}
    for full in (False, True):
        vae = LunarisCoreVAE(L)
        vae.load_state_dict(R.closed_form_params(L))
        vae = vae.to("cuda")
        t = _teacher(True)
        t.set_dropout_stream(DROP_SEED)
        w0 = {k: v.detach().clone() for k, v in t.state_dict().items()}
        st = HybridStepper(vae, t, teacher_lr=1e-4, teacher_full_backward=full, lr=1e-4)
        for s in range(3):
            st.step(x, s, R.closed_form_eps(B, L, salt=s).cuda())
        torch.cuda.synchronize()
        met = st.metrics()
        assert all(np.isfinite(v) for v in met.values()), met
        sd = t.state_dict()
        moved[full] = {k: not torch.equal(sd[k], w0[k]) for k in w0 if "running" not in k and "num_batches" not in k and "last_spatial" not in k}
    assert moved[False]["gate.2.weight"] and not moved[False]["experts.0.0.conv1.0.weight"] and not moved[False]["feature_extractor.conv1.0.weight"]
    for k, mv in moved[True].items():
        assert mv == (k.split(".")[0] not in ("semantic_head", "style_net", "prompt_net")), k


def test_module_with_full_backward_fills_every_grad_through_autograd():
    """LunarMoETeacher(full_backward=True) in a foreign training loop: `teacher_loss.backward()` (train_hybrid.py:891-904) leaves a .grad on
    every parameter on the path, equal to the reference's (fixture); multiplied by a GradScaler-style 65 536 the gradients come out
    multiplied by exactly 65 536 (the upstream normalisation is a power of two picked on the device)."""
    from lunaris_orion_amd.teacher import LunarMoETeacher
    B = 2
    x = R.normalise_sprites(R.closed_form_sprites(B)).cuda()
    z = np.load(os.path.join(GOLD, "teacher_fullgrad_drop_B2.npz"))
    grads = {}
    for scale in (1.0, 65536.0):
        m = LunarMoETeacher(num_experts=4, feature_dim=128, embedding_dim=64, dropout_rate=DROP_P, full_backward=True)
        m.load_state_dict(T.closed_form_teacher_state())
        m = m.to("cuda").train()
        m.set_dropout_stream(DROP_SEED, exact_next=True)
        out = m(x)
        loss = QW * -torch.mean(out["quality_scores"])
        (loss * scale).backward()
        torch.cuda.synchronize()
        grads[scale] = {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in m.named_parameters()}
    n = 0
    for k, g in grads[1.0].items():
        if k.split(".")[0] in ("semantic_head", "style_net", "prompt_net"):
            assert g is None, k
            continue
        assert g is not None, k
        assert torch.equal(grads[65536.0][k], g * 65536.0), k
        tag = f"tgrad/{k}"
        if tag + "/samples" not in z:
            assert g.abs().max().item() == 0.0, k         # relative-position tables
            continue
        n += 1
        g = g.cpu()
        idx = ((R.closed_form_uniform("sample." + tag, min(2048, g.numel())) + 1.0) * 0.5 * g.numel()).long().clamp_(0, g.numel() - 1)
        ref = torch.from_numpy(z[tag + "/samples"])
        ds = (g.flatten()[idx] - ref).norm().item()
        assert ds <= 4e-2 * max(ref.norm().item(), 1e-3 * float(z["total_norm"]) * (len(idx) / g.numel()) ** 0.5) + 1e-12, (k, ds, ref.norm().item())
    assert n == 210


def test_full_backward_is_bitwise_reproducible():
    """Every reduction of the full backward has a fixed order (per-block partial rows + ordered sums, one writer per k / v row in the
    attention, no float atomics): two fresh engines give bit-identical gradients, with the kept forward and with the recomputed one."""
    B = 2
    x = R.normalise_sprites(R.closed_form_sprites(B)).cuda()
    for keep in (False, True):
        runs = []
        for _ in range(2):
            got, _ = _native_grads(_teacher(True), x, True, keep)
            runs.append(got)
        for k in runs[0]:
            assert torch.equal(runs[0][k], runs[1][k]), (keep, k)


def test_full_backward_at_batch64_matches_the_oracle_on_the_device():
    """BASELINE's full batch: every gradient of the teacher's full backward at batch 64 (the shape bench.py times) against autograd of the
    oracle evaluated on the device (the same oracle/teacher_ref.py functions on ATen fp32 kernels; ~110 GB of saved activations: sized
    for the 288 GB of this GPU), default dropout on the library's masks, the step's kept forward."""
    B = 64
    x = R.normalise_sprites(R.closed_form_sprites(B))
    got, out = _native_grads(_teacher(True), x.cuda(), True, keep=True)
    torch.cuda.empty_cache()
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        ora, _ = _oracle_grads_uncached(x, True, device="cuda")
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
    torch.cuda.empty_cache()
    tot = torch.sqrt(sum((o.double() ** 2).sum() for o in ora.values() if o is not None)).item()
    worst, n = {}, 0
    for k, g in got.items():
        o = ora.get(k)
        if o is None:
            assert g.abs().max().item() == 0.0, k
            continue
        n += 1
        d, on = (g - o).norm().item(), o.norm().item()
        worst[k] = d / max(on, 1e-3 * tot)
        assert d <= 4e-2 * max(on, 1e-3 * tot), (k, d, on)
        if on >= 1e-3 * tot:
            cos = torch.nn.functional.cosine_similarity(g.flatten().double(), o.flatten().double(), dim=0).item()
            assert cos >= 0.999 and abs(g.norm().item() / on - 1.0) <= 1e-2, (k, cos, g.norm().item() / on)
    assert n == 210
    print("batch 64 worst relative errors:", sorted(worst.items(), key=lambda kv: -kv[1])[:5])


# ---- the fp16-rounding oracle (oracle/teacher_ref.py, act_dtype=torch.float16): bounds from the measured table in the module docstring ----
ROUNDED_BOUND = {"fe": 3e-3, "blk": 4e-2, "bn_ls": 2e-2, "heads": 2e-4}           # feature_dim 128, batch 2
HEADS_BOUND_FOLDED_FORWARD = 2e-2     # no dropout, production forward: the heads' inputs come from the folded feature_dim-128 path
ROUNDED_BOUND_WIDE = {"fe": 6e-3, "blk": 7e-2, "bn_ls": 2e-2, "heads": 1e-4}     # feature_dim 256, batch 1
STAT_BOUND = {"mean": 8e-4, "var": 4e-5}                                          # BatchNorm running statistics, see _stat_deviations
# twice the measured 1.3e-6 / 1.7e-5 / 1.5e-7 / 2.0e-6, but not below 16 ulp of an fp32 number of order 1 (two summation orders of a 16384-term mean)
HEAD_OUTPUT_BOUND = {"quality_scores": 3e-6, "style_embedding": 4e-5, "expert_weights": 2e-6, "semantic_score": 4e-6}
STAT_FLOOR = 4e-6      # 32 ulp of fp32: below this two fp32 sums of 16384+ terms in different orders are not told apart


def _group(k):
    """feature extractor / block conv, qkv, proj (weights and biases, shortcut conv included) / BatchNorm + layer_scale / heads + gate"""
    parts = k.split(".")
    if parts[0] == "feature_extractor":
        return "fe"
    if parts[0] != "experts":
        return "heads"
    rest = ".".join(parts[3:])
    return "bn_ls" if rest == "layer_scale" or rest.startswith(("conv1.2.", "conv2.2.", "shortcut.1.")) else "blk"


def _deviations(got, ora):
    """per tensor: (d / max(|o|, 1e-3 total), cosine, norm ratio) -- the last two None below 1e-3 of the total norm"""
    tot = torch.sqrt(sum((o.double() ** 2).sum() for o in ora.values() if o is not None)).item()
    res = {}
    for k, g in got.items():
        o = ora.get(k)
        if o is None:
            assert g.abs().max().item() == 0.0, k
            continue
        on, d = o.norm().item(), (g - o).norm().item()
        cos = ratio = None
        if on >= 1e-3 * tot:
            cos = torch.nn.functional.cosine_similarity(g.flatten().double(), o.flatten().double(), dim=0).item()
            ratio = g.norm().item() / on
        res[k] = (d / max(on, 1e-3 * tot), cos, ratio)
    return res, tot


def _worst_by_group(dev):
    w = {}
    for k, (d, _, _) in dev.items():
        if not _zero_by_construction(k) and d > w.get(_group(k), (-1.0, ""))[0]:
            w[_group(k)] = (d, k)
    return w


def _assert_rounded(dev, bound):
    """every tensor within its group's bound of the rounding oracle; the visible ones also in direction and norm, at the fp32-oracle
    tests' side conditions or what the group's bound b implies (cosine >= 1 - b^2 / 2, norm within b), whichever is tighter"""
    for k, (d, cos, ratio) in dev.items():
        if _zero_by_construction(k):
            continue
        b = bound[_group(k)]
        assert d <= b, (k, d, b)
        if cos is not None:
            assert cos >= max(0.999, 1.0 - 0.5 * b * b - 1e-7) and abs(ratio - 1.0) <= min(1e-2, b), (k, cos, ratio)


@pytest.mark.parametrize("drop,keep", [(False, False), (False, True), (True, False), (True, True)],
                         ids=["no_dropout", "no_dropout_kept_forward", "dropout_0.1", "dropout_0.1_kept_forward"])
def test_full_backward_matches_the_fp16_rounding_oracle(drop, keep):
    """Every gradient against autograd of the oracle that rounds to fp16 where the plain-form forward does (straight-through): the
    LeakyReLU kinks then fall on the same elements, and what is left is the backward's own fp16 activation gradients."""
    B = 2
    x = R.normalise_sprites(R.closed_form_sprites(B))
    got, _ = _native_grads(_teacher(drop), x.cuda(), drop, keep)
    ora, _ = _oracle_run(x, drop, act_dtype=torch.float16)[:2]
    dev, _ = _deviations(got, ora)
    assert len(dev) == 234 - 24
    print("against the rounding oracle, worst per group:", _worst_by_group(dev))
    print("against the fp32 oracle, worst per group:", _worst_by_group(_deviations(got, _oracle_grads(x, drop)[0])[0]))
    bound = dict(ROUNDED_BOUND)
    if not drop and not keep:
        bound["heads"] = HEADS_BOUND_FOLDED_FORWARD
    _assert_rounded(dev, bound)


def test_full_backward_wide_teacher_matches_the_fp16_rounding_oracle():
    """feature_dim 256 with the Conv1x1 + BatchNorm shortcut, batch 1, dropout 0.1, the step's kept (plain-form) forward; the rounding
    oracle runs on the device like the fp32 one of the test above."""
    B, F, emb = 1, 256, 256
    x = R.normalise_sprites(R.closed_form_sprites(B))
    got, _ = _native_grads(_teacher(True, F, emb), x.cuda(), True, keep=True)
    prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    try:
        ora, _ = _oracle_run(x, True, "cuda", torch.float16, feature_dim=F, embedding_dim=emb)[:2]
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
    dev, tot = _deviations(got, ora)
    assert len(dev) == 234 + 4 * 4 - 24
    for k in dev:
        if _zero_by_construction(k):
            assert ora[k].norm().item() <= 1e-4 * tot and got[k].norm().item() <= 2e-3 * tot, k
    print("feature_dim 256 against the rounding oracle, worst per group:", _worst_by_group(dev))
    _assert_rounded(dev, ROUNDED_BOUND_WIDE)


def _stat_deviations(sd, new_stats, state0):
    """per BatchNorm layer: (worst |running_mean - oracle's| in units of momentum * the batch standard deviation,
    worst |running_var - oracle's| in units of momentum * the batch variance): both are relative errors of the batch statistic.  The
    stored numbers are fp32 sums 0.9 old + 0.1 batch, so 4 ulp of the stored value are taken off first (conv2's output is close to a
    constant field, its batch variance of order 1e-5: there one ulp of running_var is percents of 0.1 * variance)."""
    res = {}
    for k, o in new_stats.items():
        if not k.endswith("running_mean"):
            continue
        p = k[:-len(".running_mean")]
        ov = new_stats[p + ".running_var"]
        var_b = ((ov - 0.9 * state0[p + ".running_var"]) / 0.1).clamp_min(1e-12)      # unbiased batch variance
        dm = ((sd[k].cpu() - o).abs() - 2.0 ** -21 * o.abs()).clamp_min(0.0)
        dv = ((sd[p + ".running_var"].cpu() - ov).abs() - 2.0 ** -21 * ov.abs()).clamp_min(0.0)
        res[p] = ((dm / (0.1 * var_b.sqrt())).max().item(), (dv / (0.1 * var_b)).max().item())
    return res


@pytest.mark.parametrize("drop", [False, True], ids=["no_dropout", "dropout_0.1"])
def test_kept_forward_batchnorm_statistics_follow_the_rounding_oracle_layer_by_layer(drop):
    """The localiser: after one train-mode plain-form forward every BatchNorm layer's running statistics (29 layers) against the
    rounding oracle's.  A rounding site the emulation misses shows at the first layer whose statistics agree no better with it than
    with the fp32 oracle."""
    B = 2
    x = R.normalise_sprites(R.closed_form_sprites(B))
    m = _teacher(drop)
    state0 = T.closed_form_teacher_state()
    if drop:
        m.set_dropout_stream(DROP_SEED, exact_next=True)
    with torch.no_grad():
        out = m._native_forward(x.cuda(), keep=True)[0]
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items() if "running" in k}
    e16, e32 = _oracle_extras(x, drop, act_dtype=torch.float16), _oracle_extras(x, drop)
    d16, d32 = _stat_deviations(sd, e16["new_stats"], state0), _stat_deviations(sd, e32["new_stats"], state0)
    assert len(d16) == 29          # 5 in the feature extractor, 2 per ExpertBlock
    for p in d16:
        print(f"{p:40s} mean {d16[p][0]:.2e} (fp32 oracle {d32[p][0]:.2e})  var {d16[p][1]:.2e} (fp32 oracle {d32[p][1]:.2e})")
    for p in d16:
        assert d16[p][0] <= STAT_BOUND["mean"] and d16[p][1] <= STAT_BOUND["var"], (p, d16[p])
        assert d16[p][0] <= max(d32[p][0], STAT_FLOOR) and d16[p][1] <= max(d32[p][1], STAT_FLOOR), (p, d16[p], d32[p])
    for k, tol in HEAD_OUTPUT_BOUND.items():
        a16, a32 = (out[k].cpu() - e16["out"][k]).abs().max().item(), (out[k].cpu() - e32["out"][k]).abs().max().item()
        print(f"{k:20s} {a16:.2e} (fp32 oracle {a32:.2e})")
        assert a16 <= tol and a16 <= a32, (k, a16, a32)
