"""The eval-mode teacher as a differentiable reward: ``LunarMoETeacher(eval_input_grad=True)`` in ``eval()`` -- the eval kept forward
(lo_teacher_forward_keep_eval) and the frozen-BatchNorm backward (lo_teacher_eval_backward) -- against autograd of the CPU oracle in
eval mode (oracle/teacher_ref.py, ``training=False``; with ``act_dtype=torch.float16`` the oracle that rounds where the plain-form
forward does), on the closed-form state (running mean +-0.05, running variance 0.75-1.25) and closed-form sprites.

Bounds.  x.grad: the project's own for the same quantities in train mode (tests/test_input_grad_gpu.py) -- fp32 oracle 8e-2 relative
L2, cosine >= 0.997, norm within 1 %, 16x16-pooled 2e-2; rounding oracle 3e-2, pooled 4e-3.  feature_dim 256 / batch 1: each times
1.75, the ratio ROUNDED_BOUND_WIDE["blk"] / ROUNDED_BOUND["blk"] (7e-2 / 4e-2) of tests/test_teacher_fullgrad_gpu.py -- the group the
images' gradient travels through; a cosine's deficit is quadratic in the deviation, so there it is 1 - 0.003 * 1.75^2.  Against the
rounding oracle the cosine bound is 1 - bound^2 / 2, as in test_teacher_input_grad_against_the_fp16_rounding_oracle.  Parameter gradients: 4e-2 per tensor as in tests/test_teacher_fullgrad_gpu.py.
Measured values: see the docstring of each test.
"""
import ctypes as C
import warnings

import pytest
import torch

from oracle import teacher_ref as T
from oracle import vae_ref as R

pytestmark = pytest.mark.gpu
QW = 0.5
KEYS = ("quality_scores", "expert_weights", "style_embedding", "prompt_embedding", "semantic_score")
FP32_BOUND = {"full": 8e-2, "pooled16": 2e-2, "cos": 0.997}
ROUNDED_BOUND = {"full": 3e-2, "pooled16": 4e-3, "cos": 1.0 - 0.5 * 3e-2 ** 2 - 1e-6}
WIDE = 7e-2 / 4e-2
PARAM_BOUND = 4e-2


def _rel(a, b):
    return (a.double() - b.double()).norm().item() / (b.double().norm().item() + 1e-30)


def _pool(a):
    return torch.nn.functional.avg_pool2d(a.double(), 16)


def _x(B):
    return R.normalise_sprites(R.closed_form_sprites(B))


def _state_kw(F, emb):
    return {} if F == 128 else {"feature_dim": F, "embedding_dim": emb}


def _teacher(F=128, emb=64, **kw):
    from lunaris_orion_amd.teacher import LunarMoETeacher
    kw.setdefault("eval_input_grad", True)
    t = LunarMoETeacher(feature_dim=F, embedding_dim=emb, **kw)            # dropout_rate: the default 0.1, which eval mode ignores
    t.load_state_dict(T.closed_form_teacher_state(**_state_kw(F, emb)))
    return t.to("cuda").eval()


def _loss(out, rows=None):
    q = out["quality_scores"]
    return QW * -torch.mean(q if rows is None else q[rows])


_ORACLE = {}


def _oracle(B, act_dtype=None, F=128, emb=64, device="cpu"):
    """{"x_grad", "grads", "out"} of the oracle's eval-mode autograd (computed once per case; the inputs are closed-form)."""
    key = (B, act_dtype, F, emb, device)
    if key not in _ORACLE:
        S = T.closed_form_teacher_state(**_state_kw(F, emb))
        P = {k: (v.to(device).clone().requires_grad_(True) if v.is_floating_point() and "running" not in k and "last_spatial" not in k else v.to(device))
             for k, v in S.items()}
        x = _x(B).to(device).clone().requires_grad_(True)
        prev = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
        torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
        try:
            out, stats = T.teacher_forward(x, P, training=False, act_dtype=act_dtype)
            names = [k for k, v in P.items() if v.requires_grad]
            g = torch.autograd.grad(_loss(out), [x] + [P[k] for k in names], allow_unused=True)
        finally:
            torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = prev
        _ORACLE[key] = {"x_grad": g[0].detach().cpu(), "grads": {k: (None if t is None else t.detach().cpu()) for k, t in zip(names, g[1:])},
                        "out": {k: v.detach().cpu() for k, v in out.items() if torch.is_tensor(v)}}
    return _ORACLE[key]


_NATIVE = {}


def _native(B, frozen, F=128, emb=64):
    """(x.grad, outputs, {name: grad}) of one forward + backward of the eval-mode module; frozen: teacher.requires_grad_(False)."""
    key = (B, frozen, F, emb)
    if key not in _NATIVE:
        t = _teacher(F, emb)
        if frozen:
            t.requires_grad_(False)
        xg = _x(B).cuda().requires_grad_()
        out = t(xg)
        _loss(out).backward()
        torch.cuda.synchronize()
        _NATIVE[key] = (xg.grad.detach().cpu(), {k: out[k].detach().cpu() for k in KEYS},
                        {k: (None if p.grad is None else p.grad.detach().cpu()) for k, p in t.named_parameters()})
    return _NATIVE[key]


def _measure(got, ref, what):
    g, r = got.double().flatten(), ref.double().flatten()
    m = {"full": _rel(got, ref), "pooled16": _rel(_pool(got), _pool(ref)),
         "cos": torch.dot(g, r).item() / (g.norm().item() * r.norm().item()), "norm": g.norm().item() / r.norm().item()}
    print(f"{what}: relative L2 {m['full']:.4e}, 16x16-pooled {m['pooled16']:.4e}, cosine {m['cos']:.6f}, norm ratio {m['norm']:.5f}")
    return m


def _assert_close(got, ref, what, bound, scale=1.0):
    """The checks of _assert_teacher_input_grad_close / test_teacher_input_grad_against_the_fp16_rounding_oracle."""
    m = _measure(got, ref, what)
    full = bound["full"] * scale
    assert m["pooled16"] <= bound["pooled16"] * scale, (what, m)
    assert m["full"] <= full, (what, m)
    assert m["cos"] >= 1.0 - (1.0 - bound["cos"]) * scale ** 2, (what, m)
    assert abs(m["norm"] - 1.0) <= 1e-2, (what, m)


# ---- 1, 2. x.grad against the reference ---------------------------------------------------------------------------------------
def test_input_grad_against_the_eval_oracles_b2_f128():
    """Measured on the MI355X: rounding oracle 4.17e-3, 16x16-pooled 8.5e-4, cosine 0.999991, norm ratio 1.00025; fp32 oracle 3.23e-2,
    2.29e-3, 0.99948, 1.00026 -- the rounding oracle's own distance to the fp32 oracle (3.2e-2 / 2.2e-3).  No starting bound exceeded."""
    got = _native(2, True)[0]
    assert torch.isfinite(got).all() and got.abs().max().item() > 0
    _assert_close(got, _oracle(2, torch.float16)["x_grad"], "x.grad, rounding oracle", ROUNDED_BOUND)
    _assert_close(got, _oracle(2)["x_grad"], "x.grad, fp32 oracle", FP32_BOUND)


def test_input_grad_against_the_eval_oracles_b1_f256():
    """The shortcut conv and its frozen BatchNorm without activation, batch-1 grids; the oracle's autograd runs on the device.
    Measured: rounding oracle 4.15e-3, pooled 5.8e-4, cosine 0.999991, norm ratio 1.00008; fp32 oracle 3.19e-2, 2.29e-3, 0.99949."""
    got = _native(1, True, 256, 64)[0]
    assert torch.isfinite(got).all() and got.abs().max().item() > 0
    _assert_close(got, _oracle(1, torch.float16, 256, 64, "cuda")["x_grad"], "F=256 x.grad, rounding oracle", ROUNDED_BOUND, WIDE)
    _assert_close(got, _oracle(1, None, 256, 64, "cuda")["x_grad"], "F=256 x.grad, fp32 oracle", FP32_BOUND, WIDE)


# ---- 3. sample independence ------------------------------------------------------------------------------------------------------
def test_samples_outside_the_loss_get_exactly_zero():
    """Frozen statistics couple no two samples (the train-mode backward does, through S1 / N and xhat S2 / N): a batch-statistic term
    left in shows here."""
    t = _teacher()
    t.requires_grad_(False)
    xg = _x(3).cuda().requires_grad_()
    _loss(t(xg), rows=[0, 2]).backward()
    g = xg.grad
    assert torch.count_nonzero(g[1]).item() == 0
    for n in (0, 2):
        assert torch.isfinite(g[n]).all() and g[n].abs().max().item() > 0, n


# ---- 4. dx-only equals with-parameters, bitwise -------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 3])
def test_dx_without_parameter_gradients_has_the_bits_of_dx_with_them(B):
    def run(frozen):
        t = _teacher()
        if frozen:
            t.requires_grad_(False)
        xg = _x(B).cuda().requires_grad_()
        _loss(t(xg)).backward()
        assert frozen == all(p.grad is None for p in t.parameters())
        return xg.grad
    live, frozen = run(False), run(True)
    assert torch.equal(live, frozen)
    assert torch.equal(run(False), live) and torch.equal(run(True), frozen)         # run to run


# ---- 5. parameter gradients ---------------------------------------------------------------------------------------------------
def _assert_first_conv_identity(x, dx, w, dw):
    """<x, dx> == <W, dW> for a bias-carrying conv whose input gradient and weight gradient come from the same dy (both equal
    <conv(x, W), dy>): pins the images' gradient to the weight gradient."""
    x, dx, w, dw = (t.detach().double().cpu() for t in (x, dx, w, dw))
    lhs, rhs = (x * dx).sum().item(), (w * dw).sum().item()
    assert abs(lhs - rhs) <= 1e-6 * (x.abs() * dx.abs()).sum().item(), (lhs, rhs)


def test_parameter_gradients_of_the_live_eval_teacher():
    """Measured worst tensor: 7.7e-4 of its norm (feature_extractor.detail_branch.0.weight; the gate's 7.4e-4 next)."""
    B = 2
    dx, _, got = _native(B, False)
    _assert_first_conv_identity(_x(B), dx, T.closed_form_teacher_state()["feature_extractor.conv1.0.weight"], got["feature_extractor.conv1.0.weight"])
    ora = _oracle(B)["grads"]
    tot = torch.sqrt(sum((o.double() ** 2).sum() for o in ora.values() if o is not None)).item()
    worst, n = {}, 0
    for k, g in got.items():
        if k.split(".")[0] in ("semantic_head", "style_net", "prompt_net"):
            assert g is None or g.abs().max().item() == 0.0, k
            continue
        assert g is not None, k
        o = ora.get(k)
        if o is None:                                   # the softmax-invariant relative-position tables
            assert g.abs().max().item() == 0.0, k
            continue
        n += 1
        on, d = o.norm().item(), (g - o).norm().item()
        worst[k] = d / max(on, 1e-3 * tot)
    print("worst relative errors:", [(k, f"{v:.3e}") for k, v in sorted(worst.items(), key=lambda kv: -kv[1])[:8]])
    assert n == 234 - 24
    bad = {k: v for k, v in worst.items() if v > PARAM_BOUND}
    assert not bad, bad
    # (that no gradient lands on running statistics is checked on the flat gradient itself: _raw_eval)


def test_frozen_batchnorm_fine_tuning_without_an_input_gradient():
    """Eval mode, full_backward=True, an input that does not require grad: lo_teacher_eval_backward with dx = NULL gives the parameter
    gradients of the run whose input requires grad, bit for bit."""
    B = 2
    t = _teacher(full_backward=True)
    x = _x(B).cuda()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = t(x)
        _loss(out).backward()
    assert not rec and x.grad is None and t.last_path(B) == 1
    ref = _native(B, False)[2]
    n = 0
    for k, p in t.named_parameters():
        assert (p.grad is None) == (ref[k] is None), k
        if p.grad is not None:
            n += 1
            assert torch.equal(p.grad.cpu(), ref[k]), k
    assert n > 200


@pytest.mark.parametrize("frozen", [True, False], ids=["dx_only", "with_parameters"])
def test_shared_tensor_set_plan_recomputes_in_eval_mode(monkeypatch, frozen):
    """The plan of scratch above 160 GB (one shared block tensor set, each block recomputed in front of its backward), forced at batch
    2 by LO_T_BWD_SHARED=1: the recomputation runs with the running statistics, so x.grad and the parameter gradients have the bits
    of the plan that keeps every tensor."""
    from lunaris_orion_amd import _lib
    B = 2
    monkeypatch.setenv("LO_T_BWD_SHARED", "1")                 # read when the engine is created
    t = _teacher()
    if frozen:
        t.requires_grad_(False)
    xg = _x(B).cuda().requires_grad_()
    _loss(t(xg)).backward()
    eng = t._engines[B]
    saved_bytes = _lib.lib.lo_teacher_full_backward_bytes(eng.handle)
    monkeypatch.delenv("LO_T_BWD_SHARED")
    ref_dx, _, ref_g = _native(B, frozen)
    assert saved_bytes < _lib.lib.lo_teacher_full_backward_bytes(_teacher()._engine(B).handle) // 2     # the shared plan it was
    assert torch.equal(xg.grad.cpu(), ref_dx)
    for k, p in t.named_parameters():
        assert (p.grad is None) == (ref_g[k] is None), k
        if p.grad is not None:
            assert torch.equal(p.grad.cpu(), ref_g[k]), k


# ---- 6. what must not move ------------------------------------------------------------------------------------------------------
def test_state_and_dropout_stream_do_not_move_and_outputs_are_the_eval_forwards():
    B = 2
    t = _teacher()
    x = _x(B).cuda()
    with torch.no_grad():
        ref = {k: v.clone() for k, v in t(x).items() if v is not None}                     # the default (folded) eval forward
    before = {k: v.detach().clone() for k, v in t.state_dict().items() if "running" in k or "num_batches" in k}
    calls, seed = t.drop_calls, t.last_drop_seed
    xg = x.clone().requires_grad_()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = t(xg)
        _loss(out).backward()
    torch.cuda.synchronize()
    assert not rec, [str(w.message) for w in rec]
    assert xg.grad is not None and t.last_path(B) == 1
    for k, v in t.state_dict().items():
        if k in before:
            assert torch.equal(v, before[k]), k
    assert t.drop_calls == calls and t.last_drop_seed == seed
    oo = _oracle(B)["out"]
    for k in KEYS:
        tol = 2e-2 if "embedding" in k else 2e-3
        assert (out[k].detach() - ref[k]).abs().max().item() <= tol, k
        assert (out[k].detach().cpu() - oo[k]).abs().max().item() <= tol, k
    assert not out["style_embedding"].requires_grad and not out["semantic_score"].requires_grad
    # the default stays what tests/test_input_grad_gpu.py pins
    d = _teacher(eval_input_grad=False)
    xd = x.clone().requires_grad_()
    with pytest.warns(UserWarning, match="eval mode"):
        d(xd)["quality_scores"].mean().backward()
    assert xd.grad is None


# ---- 7. mode handshake ----------------------------------------------------------------------------------------------------------
DROP_SEED = 0x5EEDD209C0FFEE11


def _grads(t):
    return [None if p.grad is None else p.grad.clone() for p in t.parameters()]


def _handshake(first_train, interleave):
    """forward of one mode whose input requires grad, (optionally) a whole forward + backward of the other mode on the same engine,
    then the first mode's backward.  The train-mode call in between moves the running statistics, which the eval backward's
    recomputation reads: the test puts the state back, since the handshake and not the statistics is its subject."""
    B = 2
    t = _teacher()
    t.train(first_train)
    t.set_dropout_stream(DROP_SEED, exact_next=True)
    x = _x(B).cuda()
    xa = x.clone().requires_grad_()
    la = _loss(t(xa))
    if interleave:
        flat, nbt = t._flat.clone(), t._nbt.clone()
        t.train(not first_train)
        xb = x.clone().requires_grad_()
        _loss(t(xb)).backward()
        assert xb.grad is not None
        t.zero_grad(set_to_none=True)
        t.train(first_train)
        with torch.no_grad():
            t._flat.copy_(flat)
            t._nbt.copy_(nbt)
    la.backward()
    torch.cuda.synchronize()
    return xa.grad, _grads(t)


@pytest.mark.parametrize("first_train", [True, False], ids=["train_around_eval", "eval_around_train"])
def test_a_backward_never_consumes_the_other_modes_kept_tensors(first_train):
    dx0, g0 = _handshake(first_train, False)
    dx1, g1 = _handshake(first_train, True)
    assert torch.equal(dx0, dx1)
    for a, b in zip(g0, g1):
        assert (a is None and b is None) or torch.equal(a, b)


# ---- 8, 9. raw ABI ----------------------------------------------------------------------------------------------------------------
def _raw_eval(B, fill, gscale, with_grads, keep=True, train_keep_between=False):
    """lo_teacher_forward_keep_eval + lo_teacher_eval_backward on guard-banded buffers of exactly the header's sizes, ws / bws / rows
    pre-filled with the byte `fill`, dx and the flat gradient with NaN.  Returns (dx, flat gradient or None), unscaled.
    train_keep_between: a train-mode kept forward without dropout (dropout_p 0, seed 0: what the eval forward records too) on the same
    scratch and no backward of its own in between -- only the recorded mode tells the eval backward that the tensors are not its own."""
    from lunaris_orion_amd import _lib
    from tests.guarded import check_guards, gin, guarded, written
    lib, st = _lib.lib, _lib.stream_ptr()
    t = _teacher()
    t._ensure_flat()
    h = C.c_void_p()
    _lib.check(lib.lo_teacher_create_ex(B, 4, 128, 64, 0, C.byref(h)), "create")
    try:
        flat = gin(t._flat)
        x = gin(_x(B))
        ws = guarded(lib.lo_teacher_workspace_bytes(h), torch.uint8, "ws", payload_fill=fill)
        bws = guarded(lib.lo_teacher_full_backward_bytes(h), torch.uint8, "ws", payload_fill=fill)
        _lib.check(lib.lo_teacher_pack(h, flat.data_ptr(), ws.data_ptr(), st), "pack")
        outs = [guarded(s, torch.float32, "out") for s in ((B, 4), (B, 4), (B, 64), (B, 64), (B, 1))]
        _lib.check(lib.lo_teacher_forward_keep_eval(h, x.data_ptr(), flat.data_ptr(), ws.data_ptr(), bws.data_ptr(), *[o.data_ptr() for o in outs], st),
                   "lo_teacher_forward_keep_eval")
        assert lib.lo_teacher_last_path(h) == 1
        offs, elems = (C.c_size_t * 3)(), (C.c_size_t * 3)()
        _lib.check(lib.lo_teacher_heads_saved(h, offs, elems), "saved")
        saved = [gin(ws[offs[i]:offs[i] + 4 * elems[i]].view(torch.float32).clone()) for i in range(3)]
        weights = gin(outs[1].clone())
        b, e = C.c_size_t(), C.c_size_t()
        _lib.check(lib.lo_teacher_grad_range(h, C.byref(b), C.byref(e)), "range")
        rows = guarded(B * (e.value - b.value), torch.float32, "ws", payload_fill=fill)
        # upstream of QW * -mean(quality_scores), brought to [2, 4) by a power of two like the module does (lo_grad_scale_pick)
        r = 1.0
        while QW / (B * 4) * r < 2.0:
            r *= 2.0
        dq = gin(torch.full((B, 4), -QW / (B * 4) * r))
        grads = guarded(t._flat.numel(), torch.float32, "out") if with_grads else None
        dx = guarded((B, 3, 128, 128), torch.float32, "out")
        if train_keep_between:
            flat_t = gin(t._flat)                # the train-mode forward moves the running statistics: on its own copy of the state
            _lib.check(lib.lo_teacher_forward_keep(h, x.data_ptr(), flat_t.data_ptr(), ws.data_ptr(), bws.data_ptr(), 0.0, 0,
                                                   *[o.data_ptr() for o in outs], st), "lo_teacher_forward_keep")
            assert not torch.equal(flat_t, t._flat)
        if not keep:
            bws.fill_(fill)                      # the backward does not find kept tensors: it recomputes the trunk in eval mode
            _lib.check(lib.lo_teacher_forward(h, x.data_ptr(), flat.data_ptr(), ws.data_ptr(), 0, 0.0, 0, *[o.data_ptr() for o in outs], st), "fwd")
        _lib.check(lib.lo_teacher_eval_backward(h, x.data_ptr(), flat.data_ptr(), ws.data_ptr(), bws.data_ptr(), *[s.data_ptr() for s in saved],
                                                weights.data_ptr(), dq.data_ptr(), None, float(gscale), rows.data_ptr(), _lib.ptr(grads),
                                                dx.data_ptr(), st), "lo_teacher_eval_backward")
        torch.cuda.synchronize()
        check_guards(flat, x, ws, bws, rows, dq, weights, grads, dx, *outs, *saved)
        written(dx, grads, *outs)
        assert torch.equal(flat, t._flat)                        # flat_state is const: not one byte
        if grads is not None:
            # no gradient lands on running statistics (num_batches_tracked and the other integer buffers have no slot at all)
            n_stats = 0
            for i in range(lib.lo_teacher_num_tensors(h)):
                name, off = lib.lo_teacher_tensor_name(h, i).decode(), lib.lo_teacher_tensor_offset(h, i)
                if "running_" in name:
                    n_stats += 1
                    assert off >= 0 and torch.count_nonzero(grads[off:off + lib.lo_teacher_tensor_numel(h, i)]).item() == 0, name
                elif "num_batches_tracked" in name:
                    assert off < 0, name
            assert n_stats == 2 * 29
        return dx.cpu() / r, (None if grads is None else grads.cpu() / r)
    finally:
        lib.lo_teacher_destroy(h)


@pytest.mark.parametrize("with_grads", [True, False], ids=["flat_grads", "flat_grads_null"])
def test_raw_abi_on_guarded_poisoned_memory(with_grads):
    """An unwritten kept tensor (the compact attention rows >= 543, a skipped (mean, rstd) table) would show as NaN or as other bits."""
    B = 3
    dx_ff, g_ff = _raw_eval(B, 0xFF, 2 ** 20, with_grads)
    dx_00, g_00 = _raw_eval(B, 0x00, 2 ** 20, with_grads)
    assert torch.equal(dx_ff, dx_00)
    if with_grads:
        assert torch.equal(g_ff, g_00)
    dx_re, _ = _raw_eval(B, 0xFF, 2 ** 20, with_grads, keep=False)            # recomputed trunk: the same function
    assert torch.equal(dx_re, dx_ff)


def test_eval_backward_does_not_consume_a_train_mode_kept_forward():
    """eval kept forward, then a train-mode kept forward with the same (dropout_p, seed) = (0, 0) on the same scratch, then the eval
    backward: the kept tensors are the train call's (batch statistics), and the recorded mode makes the backward recompute."""
    B = 2
    dx, g = _raw_eval(B, 0xFF, 2 ** 20, True)
    dx_t, g_t = _raw_eval(B, 0xFF, 2 ** 20, True, train_keep_between=True)
    assert torch.equal(dx, dx_t) and torch.equal(g, g_t)


def test_gscale_2p20_and_2p24():
    """The dx-only backward at both gradient scales against the rounding oracle (bounds of test 1) and against each other: the
    module's EVAL_GSCALE is the value this test supports.  Measured: 4.168e-3 / 4.168e-3 (pooled 8.506e-4 / 8.508e-4), 5.8e-5 between
    the two (pooled 4.5e-6): no underflow at 2^20."""
    from lunaris_orion_amd.teacher import EVAL_GSCALE
    ref = _oracle(2, torch.float16)["x_grad"]
    a, _ = _raw_eval(2, 0xFF, 2 ** 20, False)
    b, _ = _raw_eval(2, 0xFF, 2 ** 24, False)
    ma, mb, mab = _measure(a, ref, "gscale 2^20, rounding oracle"), _measure(b, ref, "gscale 2^24, rounding oracle"), _measure(a, b, "2^20 against 2^24")
    for m in (ma, mb, mab):
        assert m["full"] <= ROUNDED_BOUND["full"] and m["pooled16"] <= ROUNDED_BOUND["pooled16"], m
    assert EVAL_GSCALE in (2 ** 20, 2 ** 24)
    assert torch.equal(a if EVAL_GSCALE == 2 ** 20 else b, _native(2, True)[0])        # the module runs the scale tested here


# ---- 10. AMP boundary -----------------------------------------------------------------------------------------------------------
def test_fp16_input_under_autocast_with_a_loss_scale():
    """Measured against the unscaled fp32-input run: 2.98e-2, pooled 2.07e-3, cosine 0.99956 (the fp16 rounding of the images)."""
    t = _teacher()
    t.requires_grad_(False)
    xg = _x(2).cuda().half().requires_grad_()
    with torch.autocast("cuda", dtype=torch.float16):
        out = t(xg)
    (_loss(out) * 65536.0).backward()
    assert xg.grad is not None and xg.grad.dtype == xg.dtype
    got = xg.grad.float().cpu() / 65536.0
    ref = _native(2, True)[0]
    _assert_close(got, ref, "AMP x.grad / 65536 against the unscaled run", FP32_BOUND)
