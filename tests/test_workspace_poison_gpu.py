"""Whole-model runs on poisoned, guard-banded workspaces.

The header promises nothing about what a workspace holds before the first call (include/lunaris_hip.h, "What the caller provides"):
the library zeroes what it needs itself (`vae_ensure_sync_init`, `t_zero_once`, a few memsets in the steps).  A fresh allocation is
zero in practice, so a region that some kernel reads, no kernel writes and no such list names gives correct results in every other
test and garbage in a long run on recycled allocator blocks.  Here every scenario runs three times from the same seeds with the
workspace(s) pre-filled with

    zeros      what a fresh allocation looks like;
    0xFF       NaN in fp16 / fp32 / e4m3, 0xFFFFFFFF in every counter;
    0x7B       a large FINITE value in fp16 (61 280) and fp32 (1.3e36): v_max, selects and amax kernels swallow NaN, not this;

and every output, metric and gradient of the second and third run must be BITWISE equal to the first (these paths are bitwise
reproducible run to run: tests/test_vae_gpu.py::test_run_to_run_bitwise_determinism, tests/test_teacher_fullgrad_gpu.py::
test_full_backward_is_bitwise_reproducible), every guard band around every workspace intact (tests/guarded.py), and the
rendezvous-failure word 0.  Only values change: every access stays inside one allocation.  DESIGN.md ("Workspace regions: who writes
before who reads") has the audit these tests check.
"""
import functools

import pytest
import torch

from oracle import teacher_ref as T
from oracle import vae_ref as R
from tests.guarded import GUARD_BYTES, check_guards, guarded

pytestmark = pytest.mark.gpu

FILLS = (("zeros", 0x00), ("ones", 0xFF), ("x7B", 0x7B))
DROP_SEED = 0x5EEDD209C0FFEE11


# ---- the helper itself ------------------------------------------------------------------------------------------------------
def test_check_guards_names_a_stray_byte_on_either_side():
    v = guarded((3, 5), torch.float16, "out", skew=16)
    assert (v.data_ptr() - 16) % 256 == 0 and torch.isnan(v).all()
    check_guards(v)
    whole = torch.empty(0, dtype=torch.uint8, device="cuda").set_(v.untyped_storage())
    off = v.data_ptr() - whole.data_ptr()
    assert off >= GUARD_BYTES and whole.numel() - (off + 30) >= GUARD_BYTES
    whole[off + 30 + 7] = 0
    with pytest.raises(AssertionError, match=r"ABOVE .* first differing byte 7 B past the payload's end"):
        check_guards(v)
    whole[off + 30 + 7] = 0xFF
    whole[off - 3] = 1
    with pytest.raises(AssertionError, match=r"BELOW .* nearest differing byte 3 B before the payload's start"):
        check_guards(v)
    i = guarded(4, torch.int32, "out")
    assert (i.view(torch.uint8) == 0xA5).all()
    w = guarded(1000, torch.uint8, "ws", payload_fill=0x7B)
    assert (w == 0x7B).all() and w.view(torch.float16)[0].item() == 61280.0


# ---- plumbing ---------------------------------------------------------------------------------------------------------------
def _poison(monkeypatch, fill):
    """Every workspace the Python layer allocates from now on is a guarded view pre-filled with `fill`; returns the list they land in."""
    from lunaris_orion_amd import teacher as teacher_mod
    from lunaris_orion_amd import trainer as trainer_mod
    from lunaris_orion_amd import vae as vae_mod
    made = []

    def alloc(nbytes, device):
        v = guarded(int(nbytes), torch.uint8, "ws", payload_fill=fill)
        made.append(v)
        return v

    monkeypatch.setattr(vae_mod, "_alloc_workspace", alloc)
    monkeypatch.setattr(teacher_mod, "_alloc_workspace", alloc)
    monkeypatch.setattr(trainer_mod, "_alloc_scratch", alloc)
    return made


def _bits(t):
    t = t.detach().contiguous()
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype in (torch.float16, torch.bfloat16):
        return t.view(torch.int16)
    return t


def _three_runs(monkeypatch, scenario, min_workspaces=1):
    """scenario() -> {name: tensor | float | int}.  Runs it once per fill; outputs of the poisoned runs bitwise equal to the zero-filled
    run's, guards intact, sync-failure words 0."""
    results = {}
    for tag, fill in FILLS:
        made = _poison(monkeypatch, fill)
        out = scenario()
        torch.cuda.synchronize()
        assert len(made) >= min_workspaces, f"{tag}: {len(made)} workspace(s) went through the allocation functions"
        check_guards(*made)
        results[tag] = {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in out.items()}
        del out, made
        torch.cuda.empty_cache()
    ref = results["zeros"]
    for k, v in ref.items():
        if k.startswith("sync_fail"):
            for tag in results:
                assert int(results[tag][k]) == 0, f"{tag}: {k} = {int(results[tag][k])}: a fused-GroupNorm rendezvous ran out (missed counter)"
    for tag in ("ones", "x7B"):
        got = results[tag]
        assert got.keys() == ref.keys()
        for k, a in ref.items():
            b = got[k]
            if torch.is_tensor(a):
                same = a.shape == b.shape and torch.equal(_bits(a), _bits(b))
                n = "" if same or a.shape != b.shape else f" ({int((_bits(a) != _bits(b)).sum())} of {a.numel()} elements differ)"
                assert same, f"workspace pre-filled with {tag}: '{k}' is not bitwise equal to the zero-filled run{n}: stale workspace memory is read"
            else:
                assert a == b or (a != a and b != b), f"workspace pre-filled with {tag}: '{k}' = {b!r}, zero-filled run {a!r}"


@functools.lru_cache(maxsize=None)
def _vae_params(L):
    return R.closed_form_params(L)


@functools.lru_cache(maxsize=None)
def _teacher_state(F, emb):
    return T.closed_form_teacher_state() if F == 128 else T.closed_form_teacher_state(feature_dim=F, embedding_dim=emb)


@functools.lru_cache(maxsize=None)
def _images(B):
    return R.normalise_sprites(R.closed_form_sprites(B))


def _vae(L=256, precision="fp16"):
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(latent_dim=L, mfma_precision=precision)
    m.load_state_dict(_vae_params(L))
    return m.to("cuda")


def _teacher(drop, F=128, emb=64, **kw):
    from lunaris_orion_amd.teacher import LunarMoETeacher
    m = LunarMoETeacher(num_experts=4, feature_dim=F, embedding_dim=emb, dropout_rate=drop, **kw)
    m.load_state_dict(_teacher_state(F, emb))
    return m.to("cuda")


def _sync_words(m):
    return {f"sync_fail/{k}": int(e.sync_fail.item()) for k, e in m._engines.items()}


# ---- VAE --------------------------------------------------------------------------------------------------------------------
def _stepper_run(B, L=256, precision="fp16", factored=False, phased=False, steps=2):
    from lunaris_orion_amd.trainer import VAEStepper

    class Handover:                         # the phased backward (lo_vae_backward_phase 1, 3, 4) as the data-parallel path calls it
        def begin(self, g):
            pass

        def finish(self):
            pass

        def __call__(self, g):
            raise AssertionError("phased path expected")

    m = _vae(L, precision)
    x = _images(B).cuda()
    st = VAEStepper(m, lr=1e-4, min_lr=1e-6, scheduler_t0=10, weight_decay=0.01, max_grad_norm=1.0, recon_weight=1.0, kl_weight=0.1,
                    grad_sync=Handover() if phased else None)
    if not phased:
        st.linear_factored = factored
    out = {}
    for s in range(steps):                  # two steps: what step 1 leaves in the workspace is there when step 2 reads
        recon, mu, logvar = st.step(x, s, R.closed_form_eps(B, L, salt=s).cuda())
        met = st.metrics()
        out.update({f"step{s}/recon": recon, f"step{s}/mu": mu, f"step{s}/logvar": logvar})
        out.update({f"step{s}/{k}": v for k, v in met.items()})
        for i, g in enumerate(st.parameter_grads()):
            out[f"step{s}/grad{i}"] = g.clone()
    st.synchronize_parameters()
    torch.cuda.synchronize()
    out["params"] = m.flat_parameters().clone()
    out.update(_sync_words(m))
    return out


@pytest.mark.parametrize("B", [2, 5])
def test_vae_fused_steps_on_poisoned_workspace(monkeypatch, B):
    """forward + fused backward + optimizer step, twice, Linear gradients materialised."""
    _three_runs(monkeypatch, lambda: _stepper_run(B))


@pytest.mark.parametrize("B", [2, 5])
def test_vae_factored_linear_gradients_on_poisoned_workspace(monkeypatch, B):
    """lo_vae_set_linear_factored mode 1: factors, Gram matrices and the batch padding of the transposed copies live in the workspace."""
    _three_runs(monkeypatch, lambda: _stepper_run(B, factored=True))


@pytest.mark.parametrize("B", [2, 5])
def test_vae_phased_backward_on_poisoned_workspace(monkeypatch, B):
    _three_runs(monkeypatch, lambda: _stepper_run(B, phased=True, steps=1))


@pytest.mark.parametrize("B", [2, 5])
def test_vae_fp8_mode_on_poisoned_workspace(monkeypatch, B):
    """mfma_precision="fp8": e4m3 activation copies, weight scales and the fp8 pack job table are workspace regions of their own."""
    _three_runs(monkeypatch, lambda: _stepper_run(B, precision="fp8"))


@pytest.mark.parametrize("B", [2, 5])
def test_vae_autograd_path_on_poisoned_workspace(monkeypatch, B):
    def run():
        m = _vae()
        x = _images(B).cuda()
        recon, mu, logvar = m(x, R.closed_form_eps(B, 256, salt=0).cuda())
        (recon.square().mean() + mu.mean() + logvar.mean()).backward()
        torch.cuda.synchronize()
        out = {"recon": recon, "mu": mu, "logvar": logvar}
        out.update({f"grad/{k}": p.grad for k, p in m.named_parameters()})
        out.update(_sync_words(m))
        return out
    _three_runs(monkeypatch, run)


@pytest.mark.parametrize("B", [2, 5])
def test_vae_encode_decode_sample_on_poisoned_workspace(monkeypatch, B):
    def run():
        m = _vae()
        m._ensure_flat()
        x = _images(B).cuda()
        out = {}
        with torch.no_grad():
            z = R.closed_form_eps(B, 256, salt=3).cuda()
            out["decode"] = m.decode(z)                                   # first call on this workspace: no encoder has run
            mu, logvar, s0, s1, s2, _ = m._native_encode(x)
            out.update({"mu": mu, "logvar": logvar, "skip0": s0, "skip1": s1, "skip2": s2})
            for n in (1, 3):
                out[f"decode_skips{n}"] = m._native_decode(z, [s0, s1, s2][:n])[0]
            torch.manual_seed(7)
            out["sample"] = m.sample(B)
        out.update(_sync_words(m))
        return out
    _three_runs(monkeypatch, run)


# ---- teacher ----------------------------------------------------------------------------------------------------------------
def _teacher_outputs(tag, o):
    return {f"{tag}/{k}": v for k, v in o.items() if v is not None}


def _running_stats(tag, m):
    return {f"{tag}/state/{k}": v.detach().clone() for k, v in m.state_dict().items() if "running" in k}


def test_teacher_f128_forward_paths_and_heads_backward_on_poisoned_workspace(monkeypatch):
    """eval; train without dropout (sparse shortcuts: path 0); train with dropout 0.1 (every conv in full: path 2); the gate /
    quality-head gradients through the module's autograd node (lo_teacher_heads_backward_ex)."""
    B = 2

    def run():
        x = _images(B).cuda()
        out = {}
        m = _teacher(0.0).eval()
        with torch.no_grad():
            out.update(_teacher_outputs("eval", m(x)))
        m.train()
        with torch.no_grad():
            out.update(_teacher_outputs("train_p0", m(x)))
        assert m.last_path(B) == 0
        out.update(_running_stats("train_p0", m))
        for p_drop in (0.0, 0.1):
            m = _teacher(p_drop).train()
            m.set_dropout_stream(DROP_SEED, exact_next=True)
            o = m(x)
            assert m.last_path(B) == (2 if p_drop > 0 else 0)
            (0.5 * -torch.mean(o["quality_scores"]) + o["expert_weights"].square().sum()).backward()
            torch.cuda.synchronize()
            out.update(_teacher_outputs(f"train_p{p_drop}", o))
            out.update({f"train_p{p_drop}/grad/{k}": p.grad for k, p in m.named_parameters() if p.grad is not None})
            out.update(_running_stats(f"train_p{p_drop}", m))
        return out
    _three_runs(monkeypatch, run)


@pytest.mark.parametrize("keep", [False, True], ids=["recomputed", "kept_forward"])
def test_teacher_f128_full_backward_and_adamw_on_poisoned_workspace(monkeypatch, keep):
    """lo_teacher_full_backward after a plain forward (trunk recomputed into bws) and after lo_teacher_forward_keep (every block's
    output left in bws), then lo_teacher_clip_adamw_full and a forward on the re-packed operands."""
    from lunaris_orion_amd import _lib
    B = 2

    def run():
        x = _images(B).cuda()
        m = _teacher(0.1).train()
        m.set_dropout_stream(DROP_SEED, exact_next=True)
        with torch.no_grad():
            o = m._native_forward(x, keep=True)[0] if keep else m(x)
        flat = m.full_backward(x, o["expert_weights"], 0.5)
        out = _teacher_outputs("fwd", o)
        out["flat_grads"] = flat.clone()
        eng = m._engine(B)
        mm, vv = torch.zeros_like(m._flat), torch.zeros_like(m._flat)
        scratch = torch.zeros(1028, device="cuda")
        _lib.check(_lib.lib.lo_teacher_clip_adamw_full(eng.handle, m._flat.data_ptr(), flat.data_ptr(), mm.data_ptr(), vv.data_ptr(), 0.05, 1e-3,
                                                       0.9, 0.999, 1e-8, 0.01, 1, scratch.data_ptr(), _lib.stream_ptr()), "clip_adamw_full")
        m.mark_weights_changed()
        m.set_dropout_stream(DROP_SEED + 1, exact_next=True)
        with torch.no_grad():
            out.update(_teacher_outputs("after_update", m(x)))
        out["scratch"] = scratch[1024:1028].clone()
        out["state"] = m._flat.clone()
        return out
    _three_runs(monkeypatch, run, min_workspaces=3)       # ws, bws and the head-gradient rows


def test_teacher_f256_forward_and_full_backward_on_poisoned_workspace(monkeypatch):
    """feature_dim 256: the shortcut branch and the compacted attention rows (`o_attc`, zeroed once per workspace)."""
    B = 2

    def run():
        x = _images(B).cuda()
        m = _teacher(0.1, F=256, emb=256).train()
        m.set_dropout_stream(DROP_SEED, exact_next=True)
        with torch.no_grad():
            o = m(x)
        flat = m.full_backward(x, o["expert_weights"], 0.5)
        out = _teacher_outputs("fwd", o)
        out["flat_grads"] = flat.clone()
        out.update(_running_stats("fwd", m))
        return out
    _three_runs(monkeypatch, run, min_workspaces=3)


def test_teacher_f512_forward_on_poisoned_workspace(monkeypatch):
    B = 1

    def run():
        x = _images(B).cuda()
        m = _teacher(0.1, F=512, emb=256).eval()
        out = {}
        with torch.no_grad():
            out.update(_teacher_outputs("eval", m(x)))
            m.train()
            m.set_dropout_stream(DROP_SEED, exact_next=True)
            out.update(_teacher_outputs("train", m(x)))
        out.update(_running_stats("train", m))
        return out
    _three_runs(monkeypatch, run)


# ---- hybrid -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("full", [False, True], ids=["heads_only", "teacher_full_backward"])
def test_hybrid_step_on_poisoned_workspaces(monkeypatch, full):
    """One HybridStepper step: VAE + teacher + reward; the stepper's own scratch (head-gradient rows, the teacher's bws) poisoned too."""
    from lunaris_orion_amd.trainer import HybridStepper
    B, L = 2, 256

    def run():
        vae = _vae(L)
        t = _teacher(0.1).train()
        t.set_dropout_stream(0x5EED0F8)
        st = HybridStepper(vae, t, lr=1e-4, teacher_lr=1e-4, teacher_full_backward=full)
        recon, mu, logvar = st.step(_images(B).cuda(), 0, R.closed_form_eps(B, L, salt=0).cuda())
        met = st.metrics()
        st.synchronize_parameters()
        torch.cuda.synchronize()
        out = {"recon": recon, "mu": mu, "logvar": logvar, "vae_params": vae.flat_parameters().clone(), "teacher_state": t._flat.clone(),
               "teacher_grads": st.t_grads.clone()}
        out.update({f"metric/{k}": v for k, v in met.items()})
        out.update(_teacher_outputs("teacher", st.last_teacher_out))
        out.update(_sync_words(vae))
        return out
    _three_runs(monkeypatch, run, min_workspaces=4 if full else 3)      # VAE ws, teacher ws, rows (+ bws)
