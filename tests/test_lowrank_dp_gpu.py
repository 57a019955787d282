"""Data parallel, mode 3 of lo_vae_set_linear_factored (csrc/lo_lowrank.hip): the ranks all-gather the Linear layers' factors and the
averaged weight gradients of fc_mu | fc_logvar and decoder.fc are never written -- clip_grad_norm_'s share (train_hybrid.py:913)
comes from Gram matrices over the combined batch axis of all ranks, AdamW (train_hybrid.py:921) forms every gradient tile from the
gathered blocks.  The reference has no distributed code; what is checked is the project's own identity: the same update as mode 2
(gathered factors materialised, then the ordinary passes) and as an fp64 evaluation of the same fp16 factors.
  1. op level, through the C ABI on guard-banded buffers of exactly the stated sizes: gradient tiles (via the moments), norm,
     operand copies, the skip on a non-finite norm, determinism;
  2. model level: "ranks" one after the other on this GPU, mode 3 against mode 2, serial and pipelined;
  3. the real exchange object (one-rank RCCL group): the norm call on the communication stream, the gathered buffer reused across steps;
  4. the fallback above world * padded batch = 512.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import vae_ref as R
from tests.guarded import check_guards, gin, guarded, written
from tests.stepper_scenarios import _OneGpuRanks

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS, WD, STEP = 1e-4, 0.9, 0.999, 1e-8, 0.01, 3
K = 192                                # three 64-column bands; N = 128 (two row tiles, non-square) unless a case says otherwise


def _bp(B):
    return (B + 31) // 32 * 32


def _op_case(B, world, N, seed=0):
    """Random fp16 factors of `world` ranks in the gathered block layout (rank r at r * rstride, transposed, batch-padded with zeros;
    whatever lies between the factors is NaN) and the fp64 gradient sum_r dY_r^T X_r of the same fp16 values."""
    g = torch.Generator().manual_seed(1000 * B + world + 7 * N + seed)
    Bp = _bp(B)
    rstride = (N + K) * Bp
    yt = torch.full(((world - 1) * rstride + N * Bp,), float("nan"), dtype=torch.float16)
    xt = torch.full(((world - 1) * rstride + K * Bp,), float("nan"), dtype=torch.float16)
    grad = torch.zeros(N, K, dtype=torch.float64)
    for r in range(world):
        dy = torch.randn(B, N, generator=g).half()
        x = torch.randn(B, K, generator=g).half()
        blk = torch.zeros(N, Bp, dtype=torch.float16)
        blk[:, :B] = dy.t()
        yt[r * rstride:r * rstride + N * Bp] = blk.reshape(-1)
        blk = torch.zeros(K, Bp, dtype=torch.float16)
        blk[:, :B] = x.t()
        xt[r * rstride:r * rstride + K * Bp] = blk.reshape(-1)
        grad += dy.double().t() @ x.double()
    p = 0.02 * torch.randn(N, K, generator=g)
    m = 0.01 * torch.randn(N, K, generator=g)
    v = 1e-4 * torch.rand(N, K, generator=g)
    return xt, yt, rstride, grad, p, m, v


def _adamw_ref(p, g, m, v):
    """lo_adamw_elem_lr in fp64 (clip coefficient 1)."""
    p, m, v = p.double(), m.double(), v.double()
    bc1, bc2s = 1.0 - B1 ** STEP, (1.0 - B2 ** STEP) ** 0.5
    m2 = m + (g - m) * (1.0 - B1)
    v2 = (1.0 - B2) * g * g + v * B2
    p2 = p * (1.0 - LR * WD) - (LR / bc1) * m2 / (v2.sqrt() / bc2s + EPS)
    return p2, m2, v2


def _run_adamw(xt, yt, rstride, world, B, gscale, p, m, v, finite=1.0):
    from lunaris_orion_amd import _lib
    N = p.shape[0]
    bufs = dict(p=gin(p), m=gin(m), v=gin(v), cast=guarded((N, K), torch.float16, "out"), cast_t=guarded((K, N), torch.float16, "out"),
                xt=gin(xt), yt=gin(yt), norm=gin(torch.tensor([0.5, 1.0, finite])))
    _lib.check(_lib.lib.lo_lowrank_gathered_adamw(bufs["p"].data_ptr(), bufs["m"].data_ptr(), bufs["v"].data_ptr(), bufs["cast"].data_ptr(),
                                                  bufs["cast_t"].data_ptr(), bufs["xt"].data_ptr(), bufs["yt"].data_ptr(), rstride, world, N, K, B,
                                                  gscale, bufs["norm"].data_ptr(), LR, B1, B2, EPS, WD, STEP, _lib.stream_ptr()),
               "lo_lowrank_gathered_adamw")
    torch.cuda.synchronize()
    check_guards(*bufs.values())
    return bufs


def _run_sumsq(xt, yt, rstride, world, B, N, scale):
    from lunaris_orion_amd import _lib
    nbytes = _lib.lib.lo_lowrank_gathered_scratch_bytes(world, B)
    assert nbytes == 4 * (world * _bp(B)) ** 2
    gram = guarded(nbytes // 4, torch.float32, "ws")
    partial = guarded(128, torch.float32, "out")
    gx, gy = gin(xt), gin(yt)
    _lib.check(_lib.lib.lo_lowrank_gathered_sumsq(gy.data_ptr(), N, gx.data_ptr(), K, rstride, world, B, scale, gram.data_ptr(),
                                                  partial.data_ptr(), _lib.stream_ptr()), "lo_lowrank_gathered_sumsq")
    torch.cuda.synchronize()
    check_guards(gram, partial, gx, gy)
    written(partial)                   # every slot
    return partial


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("B,world,N", [(1, 1, 128), (33, 2, 128), (33, 3, 128), (64, 8, 128), (64, 8, 1088), (64, 3, 320)],
                         ids=["b1_w1", "b33_w2", "b33_w3", "b64_w8", "b64_w8_n1088", "b64_w3_n320"])
def test_gathered_tiles_norm_and_copies_match_fp64(B, world, N):
    """Zero-padded batch columns (1, 33), an odd rank count, a combined contraction of 3 * 64 = 192 (six MFMA K steps from an odd rank
    count) and the 512 limit.  N = 1088 at the limit: 17 row tiles, so above a combined contraction of 256 -- where a workgroup has 8
    waves with two row tiles each -- the first workgroup of a band gives every wave a second tile (groups 4..7: the second tile's rows,
    the p / m / v double buffer rolling over, the transposed-copy staging reused) and the second workgroup has one wave with a single
    tile and seven with none.  N = 320 at a contraction of 192: five tiles on the 4-wave form, a second workgroup with one live wave."""
    xt, yt, rstride, grad, p, m, v = _op_case(B, world, N)
    gscale = 1.0 / 1024.0
    g = grad * gscale
    # the norm: the project's figure for the Gram norm against the materialised one
    partial = _run_sumsq(xt, yt, rstride, world, B, N, gscale)
    got, ref = partial.double().sum().item(), (g * g).sum().item()
    print(f"sumsq B={B} world={world}: got {got:.9e} ref {ref:.9e} rel {abs(got - ref) / ref:.2e}")
    assert abs(got - ref) <= 2e-5 * ref, (got, ref)
    # the update from the fp64 gradient: "same fp16 products, fp32 accumulation in another order" (2e-6), doubled for the square
    out = _run_adamw(xt, yt, rstride, world, B, gscale, p, m, v)
    pr, mr, vr = _adamw_ref(p, g, m, v)
    dm = (out["m"].cpu().double() - mr).norm().item() / mr.norm().item()
    dv = (out["v"].cpu().double() - vr).norm().item() / vr.norm().item()
    dp = (out["p"].cpu().double() - pr).abs()
    print(f"adamw B={B} world={world}: dm {dm:.2e} dv {dv:.2e} dp max {dp.max().item():.2e} mean {dp.mean().item():.2e}")
    assert dm <= 2e-6 and dv <= 4e-6, (dm, dv)
    assert dp.max().item() <= 2.5 * LR and dp.mean().item() <= 0.02 * LR, (dp.max().item(), dp.mean().item())
    assert torch.equal(_bits(out["cast"]), _bits(out["p"].half()))
    assert torch.equal(_bits(out["cast_t"]), _bits(out["cast"].t()))
    # the same call twice: the same bits
    again = _run_adamw(xt, yt, rstride, world, B, gscale, p, m, v)
    for k in ("p", "m", "v", "cast", "cast_t"):
        assert torch.equal(_bits(out[k]), _bits(again[k])), k
    assert torch.equal(_bits(partial), _bits(_run_sumsq(xt, yt, rstride, world, B, N, gscale)))
    # a non-finite norm (norm[2] == 0): nothing is touched
    skipped = _run_adamw(xt, yt, rstride, world, B, gscale, p, m, v, finite=0.0)
    for k, t in (("p", p), ("m", m), ("v", v)):
        assert torch.equal(_bits(skipped[k].cpu()), _bits(t)), k
    for k in ("cast", "cast_t"):
        assert bool((_bits(skipped[k]) == -1).all()), k              # still the all-ones sentinel


# ---- model level ----------------------------------------------------------------------------------------------------------------
_LIN = ("encoder.fc_mu.weight", "encoder.fc_logvar.weight", "decoder.fc.weight")


def _stepper(L, **kw):
    from lunaris_orion_amd.trainer import VAEStepper
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(L)
    m.load_state_dict(R.closed_form_params(L))
    m = m.to("cuda")
    return m, VAEStepper(m, **kw)


def _shards(L, Bper, world):
    x = R.normalise_sprites(R.closed_form_sprites(Bper * world)).cuda()
    eps = R.closed_form_eps(Bper * world, L, salt=0).cuda()
    return [(x[r * Bper:(r + 1) * Bper].contiguous(), eps[r * Bper:(r + 1) * Bper].contiguous()) for r in range(world)]


@functools.lru_cache(maxsize=None)
def _gathered_blocks(L, Bper, world):
    """Pass 1: every rank's factor block, rank-major: what the all-gather delivers.  Computed once, never modified."""
    blocks = []
    for xs, es in _shards(L, Bper, world):
        col = _OneGpuRanks(world)
        _, st = _stepper(L, lr=0.0, weight_decay=0.0, max_grad_norm=1e9, grad_sync=col, dp_factored_adamw=False)
        st.step(xs, 0, es)
        torch.cuda.synchronize()
        blocks.append(col.block)
    return torch.cat(blocks)


@pytest.mark.parametrize("pipelined", [False, True], ids=["serial", "pipelined"])
@pytest.mark.parametrize("Bper,world", [(2, 2), (1, 3)])
def test_mode3_step_equals_mode2_step(Bper, world, pipelined):
    from lunaris_orion_amd import _lib
    L, lr = 64, 1e-4
    gathered = _gathered_blocks(L, Bper, world)
    shards = _shards(L, Bper, world)
    res = {}
    for on in (False, True):
        for r, (xs, es) in enumerate(shards):
            m, st = _stepper(L, lr=lr, max_grad_norm=1e9, pipeline_optimizer=pipelined, grad_sync=_OneGpuRanks(world, gathered.clone()),
                             dp_factored_adamw=on)
            st.grads.fill_(float("nan"))
            st.step(xs, 0, es)
            st.synchronize_parameters()
            torch.cuda.synchronize()
            eng = m._engine(Bper)
            lin = [(o, n, k) for (o, n, _), (k, _) in zip(m._layout, m.named_parameters()) if k in _LIN]
            assert len(lin) == 3
            for o, n, k in lin:
                if on:
                    assert torch.isnan(st.grads[o:o + n]).all(), k        # nothing materialised the averaged matrices
                else:
                    assert torch.isfinite(st.grads[o:o + n]).all(), k
            assert _lib.lib.lo_vae_linear_factored(eng.handle) == (3 if on else 0) and eng.fac_mode == (3 if on else 2)
            gn = st.metrics()["grad_norm"]
            with torch.no_grad():
                recon, mu, _ = m(xs, R.closed_form_eps(Bper, L, salt=9).cuda())     # reads the fp16 copies and transposed copies the pass wrote
            grads = {k: g.clone() for (k, _), g in zip(m.named_parameters(), st.parameter_grads()) if k in _LIN}
            res[on, r] = dict(p=m.flat_parameters().clone(), m=st.exp_avg.clone(), v=st.exp_avg_sq.clone(), gn=gn, recon=recon.clone(),
                              mu=mu.clone(), grads=grads, lin=lin)
    for r in range(world):
        a, b = res[False, r], res[True, r]
        mask = torch.zeros_like(a["p"], dtype=torch.bool)
        for o, n, k in a["lin"]:
            mask[o:o + n] = True
            dp = (b["p"][o:o + n] - a["p"][o:o + n]).abs()
            assert dp.max().item() <= 2.5 * lr and dp.mean().item() <= 0.02 * lr, (k, dp.max().item(), dp.mean().item())
            for w in ("m", "v"):
                d = (b[w][o:o + n] - a[w][o:o + n]).norm().item() / a[w][o:o + n].norm().item()
                assert d <= 1e-4, (k, w, d)
            d = (b["grads"][k].double() - a["grads"][k].double()).norm().item() / a["grads"][k].double().norm().item()
            assert d <= 2e-6, (k, d)
        for w in ("p", "m", "v"):
            assert torch.equal(a[w][~mask], b[w][~mask]), w                     # every other parameter: the same launches
        assert abs(a["gn"] - b["gn"]) <= 2e-5 * a["gn"], (a["gn"], b["gn"])
        assert (a["recon"] - b["recon"]).abs().max().item() <= 5e-3 and (a["mu"] - b["mu"]).abs().max().item() <= 5e-3
    # every rank forms the same bits from the same gathered buffer
    for o, n, k in res[True, 0]["lin"]:
        assert torch.equal(res[True, 0]["p"][o:o + n], res[True, 1]["p"][o:o + n]), k


def test_mode3_through_the_rccl_exchange_equals_the_single_process_factored_step():
    """One-rank RCCL group, FlatGradSync(force=True): three pipelined steps at B = 4, L = 64 in mode 3 against the single-process
    factored stepper (mode 1).  With one rank the averaged gradient IS the rank's.  The norm of every step is held to the Gram-norm
    figure (2e-5), the losses, parameters and moments to the figures of test_factored_optimizer_steps_equal_the_materialised_path."""
    import os
    import subprocess
    import sys
    code = r"""
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, %r)
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", WORLD_SIZE="1")
torch.cuda.set_device(0)
dist.init_process_group("nccl", rank=0, world_size=1)
from oracle import vae_ref as R
from lunaris_orion_amd.vae import LunarisCoreVAE
from lunaris_orion_amd.trainer import VAEStepper
from lunaris_orion_amd.parallel import FlatGradSync
L, B, lr = 64, 4, 1e-4
P = R.closed_form_params(L)
xs = [R.normalise_sprites(R.closed_form_sprites(B, salt=s)).cuda() for s in range(2)]
res = []
for dp in (False, True):
    sync = FlatGradSync(force=True) if dp else None
    m = LunarisCoreVAE(L); m.load_state_dict(P); m = m.to("cuda")
    st = VAEStepper(m, lr=lr, max_grad_norm=1.0, pipeline_optimizer=True, grad_sync=sync, dp_factored_adamw=dp)
    trace = []
    for s in range(3):
        st.step(xs[s %% 2], s, R.closed_form_eps(B, L, salt=s).cuda())
        met = st.metrics()
        trace.append((met["recon_loss"], met["kl_loss"], met["grad_norm"], met["grads_finite"]))
    st.synchronize_parameters()
    torch.cuda.synchronize()
    assert m._engine(B).fac_mode == (3 if dp else 1), m._engine(B).fac_mode
    if dp:
        assert sync.modes_per_phase()[0] == "factors", sync.modes_per_phase()
    res.append((trace, m.flat_parameters().clone(), st.exp_avg.clone(), st.exp_avg_sq.clone()))
(ta, pa, ma, va), (tb, pb, mb, vb) = res
for a, b in zip(ta, tb):
    print("norm", a[2], b[2], abs(a[2] - b[2]) / a[2], "recon", a[0], b[0], "kl", a[1], b[1])
for a, b in zip(ta, tb):
    assert a[3] == 1.0 and b[3] == 1.0, (ta, tb)
    assert abs(a[0] - b[0]) <= 2e-5 * abs(a[0]) and abs(a[1] - b[1]) <= 2e-4 * abs(a[1]) and abs(a[2] - b[2]) <= 2e-5 * a[2], (ta, tb)
d = (pa - pb).abs()
assert d.max().item() <= 2.5 * 3 * lr and d.mean().item() <= 0.02 * lr, (d.max().item(), d.mean().item())
dm = (ma - mb).norm().item() / ma.norm().item()
dv = (va - vb).norm().item() / va.norm().item()
assert dm <= 1e-4 and dv <= 1e-4, (dm, dv)
dist.destroy_process_group()
print("MODE3_RCCL_OK")
""" % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "MODE3_RCCL_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


def test_above_the_combined_rank_limit_the_ops_refuse_and_the_stepper_stays_in_mode_2():
    from lunaris_orion_amd import _lib
    assert _lib.lib.lo_lowrank_gathered_scratch_bytes(16, 64) == 0 and _lib.lib.lo_lowrank_gathered_scratch_bytes(8, 64) == 4 * 512 * 512
    t = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")        # never touched: the calls are refused before any launch
    d = t.data_ptr()
    rc = _lib.lib.lo_lowrank_gathered_adamw(d, d, d, None, None, d, d, 256 * 64, 16, 64, 64, 64, 1.0, None, LR, B1, B2, EPS, WD, 1, _lib.stream_ptr())
    assert rc == -1 and b"512" in _lib.lib.lo_last_error(), _lib.lib.lo_last_error()
    rc = _lib.lib.lo_lowrank_gathered_sumsq(d, 64, d, 64, 256 * 64, 5, 128, 1.0, d, d, _lib.stream_ptr())
    assert rc == -1 and b"512" in _lib.lib.lo_last_error(), _lib.lib.lo_last_error()
    # ... and what the header forbids: a rank stride that breaks the 16-byte loads, a misaligned factor, a transpose off the 64 grid
    rc = _lib.lib.lo_lowrank_gathered_adamw(d, d, d, None, None, d, d, 12, 2, 64, 64, 64, 1.0, None, LR, B1, B2, EPS, WD, 1, _lib.stream_ptr())
    assert rc == -1 and b"multiple of 8" in _lib.lib.lo_last_error(), _lib.lib.lo_last_error()
    rc = _lib.lib.lo_lowrank_gathered_sumsq(d, 64, d, 64, 12, 2, 64, 1.0, d, d, _lib.stream_ptr())
    assert rc == -1 and b"multiple of 8" in _lib.lib.lo_last_error(), _lib.lib.lo_last_error()
    rc = _lib.lib.lo_lowrank_gathered_sumsq(d + 2, 64, d, 64, 256 * 64, 2, 64, 1.0, d, d, _lib.stream_ptr())
    assert rc == -1 and b"aligned" in _lib.lib.lo_last_error(), _lib.lib.lo_last_error()
    assert _lib.lib.lo_transpose_f16(d, d + 4096, 100, 64, _lib.stream_ptr()) == -1 and b"multiples of 64" in _lib.lib.lo_last_error()
    torch.cuda.synchronize()
    assert float(t.abs().max()) == 0.0
    m, st = _stepper(64, grad_sync=_OneGpuRanks(16), dp_factored_adamw=True)
    eng = m._engine(64)
    assert _lib.lib.lo_vae_gathered_scratch_bytes(eng.handle, 16) == 0 and _lib.lib.lo_vae_gathered_scratch_bytes(eng.handle, 8) == 2 * 4 * 512 * 512
    assert st._dp_linear_mode(eng, True, True) == 2                      # 16 x 64 = 1024 > 512
    st.grad_sync.world = 8
    assert st._dp_linear_mode(eng, True, True) == 3
    assert st._dp_linear_mode(eng, True, False) == 2                     # no `then` hook behind the exchange: nothing could take the norm
    st.dp_factored_adamw = False
    assert st._dp_linear_mode(eng, True, True) == 2
    rc = _lib.lib.lo_vae_gathered_early_norm(eng.handle, d, 8, d, d, d, _lib.stream_ptr())
    assert rc == -3 and b"mode 3" in _lib.lib.lo_last_error()            # the engine is not in mode 3
