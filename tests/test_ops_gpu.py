"""GPU parity tests of the single HIP ops (through the C ABI) against plain PyTorch fp32 on the CPU.

Inputs are rounded through fp16 first (the kernels' operand type), so the only differences left are
fp32 accumulation order and the fp16 rounding of the outputs; tolerances are stated per test.
"""
import pytest
import torch
import torch.nn.functional as F

from tests.guarded import check_guards, gin, guarded, written
from tests.hip_helpers import L, conv_forward, conv_wgrad, from_nhwc, h16, rel_err, sync

# Every device buffer a kernel sees comes from tests/guarded.py: exactly the size the ABI states, a NaN / sentinel guard band of
# 1 MiB on each side, checked bit for bit after the existing assertions.  The *_aligned16 tests run one case of each op with every
# pointer at (256 B multiple) + 16 B: the alignment include/lunaris_hip.h promises, not the 512 B of torch's allocator.

pytestmark = pytest.mark.gpu

KIND_S1, KIND_S2, KIND_T4, KIND_S1D, KIND_S2D, KIND_T4D, KIND_LIN = range(7)


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return h16(torch.randn(*shape, generator=g) * scale)


CONV_CASES = [
    # kind, B, Cin, Cout, H
    (KIND_S1, 2, 64, 64, 64),
    (KIND_S1, 2, 128, 128, 32),
    (KIND_S1, 3, 512, 512, 8),
    (KIND_S1, 8, 256, 256, 16),
    (KIND_S2, 2, 64, 128, 64),
    (KIND_S2, 2, 256, 512, 16),
    (KIND_T4, 2, 512, 256, 8),
    (KIND_T4, 2, 64, 32, 64),
    (KIND_T4, 4, 128, 64, 32),
]


def _nhwc_h(x_nchw, skew=0):
    """fp32 NCHW (CPU) -> guarded fp16 NHWC input on the GPU."""
    return gin(x_nchw.permute(0, 2, 3, 1), skew, torch.float16)


@pytest.mark.parametrize("kind,B,Cin,Cout,H", CONV_CASES)
def test_conv_forward_and_gn_partials(kind, B, Cin, Cout, H):
    _conv_forward_and_gn_partials(kind, B, Cin, Cout, H)


def _conv_forward_and_gn_partials(kind, B, Cin, Cout, H, skew=0):
    x = _rand(B, Cin, H, H, seed=1)
    if kind == KIND_T4:
        w = _rand(Cin, Cout, 4, 4, seed=2, scale=(Cin * 4) ** -0.5)
        ref = F.conv_transpose2d(x, w, None, stride=2, padding=1)
    else:
        w = _rand(Cout, Cin, 3, 3, seed=2, scale=(Cin * 9) ** -0.5)
        ref = F.conv2d(x, w, None, stride=1 if kind == KIND_S1 else 2, padding=1)
    bias = _rand(Cout, seed=3, scale=0.1)
    ref = ref + bias.view(1, -1, 1, 1)
    out, part, mt = conv_forward(kind, x, w, bias, Cout, want_partial=True, skew=skew)
    got = from_nhwc(out)
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item()
    assert err <= 4e-3 * max(1.0, ref.abs().max().item()), err   # fp16 output rounding (2^-11 relative)
    # GroupNorm partial sums: (sum, sumsq) per (sample, group) of the fp16-rounded output
    G = Cout // 8
    tot = part.double().sum(dim=1).cpu()                            # [B, 8, 2]
    g5 = got.double().view(B, 8, G, -1)
    assert torch.allclose(tot[:, :, 0], g5.sum(dim=(2, 3)), rtol=1e-4, atol=1e-2)
    assert torch.allclose(tot[:, :, 1], (g5 * g5).sum(dim=(2, 3)), rtol=1e-4, atol=1e-2)


DGRAD_CASES = [
    (KIND_S1D, KIND_S1, 2, 64, 64, 64),
    (KIND_S1D, KIND_S1, 2, 512, 512, 8),
    (KIND_S2D, KIND_S2, 2, 64, 128, 64),
    (KIND_S2D, KIND_S2, 32, 64, 128, 64),      # batch >= 32: the patch-resident form (all four phases from one dy patch)
    (KIND_S2D, KIND_S2, 2, 256, 512, 16),
    (KIND_T4D, KIND_T4, 2, 512, 256, 8),
    (KIND_T4D, KIND_T4, 2, 64, 32, 64),
]


@pytest.mark.parametrize("dkind,fkind,B,Cin,Cout,H", DGRAD_CASES)
def test_conv_dgrad(dkind, fkind, B, Cin, Cout, H):
    """data gradient == autograd of the forward op; also exercises the fused residual add."""
    _conv_dgrad(dkind, fkind, B, Cin, Cout, H)


def _conv_dgrad(dkind, fkind, B, Cin, Cout, H, skew=0):
    x = _rand(B, Cin, H, H, seed=1).requires_grad_(True)
    if fkind == KIND_T4:
        w = _rand(Cin, Cout, 4, 4, seed=2, scale=(Cin * 4) ** -0.5)
        y = F.conv_transpose2d(x, w, None, stride=2, padding=1)
    else:
        w = _rand(Cout, Cin, 3, 3, seed=2, scale=(Cin * 9) ** -0.5)
        y = F.conv2d(x, w, None, stride=1 if fkind == KIND_S1 else 2, padding=1)
    dy = _rand(*y.shape, seed=4)
    (dx_ref,) = torch.autograd.grad(y, x, dy)
    add = _rand(*x.shape, seed=5)
    # the dgrad op reads dy (channels = Cout of the forward) and writes Cin channels
    out = conv_forward(dkind, dy, w, None, Cin, add_src=add, skew=skew)
    got = from_nhwc(out)
    ref = dx_ref + add
    err = (got - ref).abs().max().item()
    assert err <= 4e-3 * max(1.0, ref.abs().max().item()), err


WGRAD_CASES = [
    (KIND_S1, 2, 64, 64, 64),
    (KIND_S1, 4, 512, 512, 8),
    (KIND_S1, 2, 128, 128, 32),
    (KIND_S1, 3, 256, 256, 16),          # multi-tap kernel: odd batch (uneven pixel splits)
    (KIND_S1, 1, 64, 128, 16),           # ... Cin != Cout
    (KIND_S1, 5, 128, 64, 8),            # ... 8-pixel-wide maps (4x8 chunks)
    (KIND_S2, 2, 64, 128, 64),
    (KIND_S2, 2, 256, 512, 16),
    (KIND_T4, 2, 512, 256, 8),
    (KIND_T4, 2, 64, 32, 64),
    (KIND_T4, 2, 128, 64, 32),
    (KIND_S2, 3, 128, 256, 32),          # stride-2 multi-tap kernel: odd batch (uneven chunk splits)
    (KIND_S2, 1, 64, 128, 16),           # ... a single 8x8 coarse map (two chunks)
    (KIND_T4, 3, 256, 128, 16),
    (KIND_T4, 1, 64, 32, 8),             # ... 32 output channels: half of the F tile is padding
    (KIND_T4, 5, 64, 64, 8),
    (KIND_S1, 7, 128, 128, 32),          # multi-tap kernel: the slab is sized for 42 splits, 38 are launched and written
]


@pytest.mark.parametrize("kind,B,Cin,Cout,H", WGRAD_CASES)
def test_conv_wgrad(kind, B, Cin, Cout, H):
    _conv_wgrad(kind, B, Cin, Cout, H)


def _conv_wgrad(kind, B, Cin, Cout, H, skew=0):
    x = _rand(B, Cin, H, H, seed=1)
    if kind == KIND_T4:
        w = _rand(Cin, Cout, 4, 4, seed=2).requires_grad_(True)
        y = F.conv_transpose2d(x, w, None, stride=2, padding=1)
    else:
        w = _rand(Cout, Cin, 3, 3, seed=2).requires_grad_(True)
        y = F.conv2d(x, w, None, stride=1 if kind == KIND_S1 else 2, padding=1)
    dy = _rand(*y.shape, seed=4, scale=0.1)
    (dw_ref,) = torch.autograd.grad(y, w, dy)
    got = conv_wgrad(kind, x, dy, Cout, tuple(w.shape), scale=0.5, skew=skew)
    assert torch.isfinite(got).all()
    assert rel_err(got, 0.5 * dw_ref) <= 2e-4, rel_err(got, 0.5 * dw_ref)   # fp32 accumulate of exact fp16 products


@pytest.mark.parametrize("M,K,N,nsplit", [(2, 32768, 512, 32), (64, 32768, 1024, 32), (8, 512, 128, 4), (37, 1024, 64, 3)])
def test_linear_splitk(M, K, N, nsplit):
    _linear_splitk(M, K, N, nsplit)


def _linear_splitk(M, K, N, nsplit, skew=0, slab_short=0):
    lib = L()
    x = _rand(M, K, seed=1)
    w = _rand(N, K, seed=2, scale=K ** -0.5)
    b = _rand(N, seed=3)
    ref = F.linear(x, w, b)
    xd = gin(x, skew, torch.float16)
    wd = gin(w, skew, torch.float16)
    slab = guarded((nsplit - slab_short) * M * N, torch.float32, "out", skew)   # the header's size: nsplit*M*N floats
    out = guarded((M, N), torch.float32, "out", skew)
    bdev = gin(b, skew)   # keep device copies alive until the kernels have run
    lib.check(lib.lib.lo_linear_splitk(M, K, N, xd.data_ptr(), wd.data_ptr(), bdev.data_ptr(), slab.data_ptr(), nsplit,
                                       out.data_ptr(), None, lib.stream_ptr()))
    sync()
    assert (out.cpu() - ref).abs().max().item() <= 2e-4 * max(1.0, ref.abs().max().item())
    check_guards(xd, wd, slab, out, bdev)


@pytest.mark.parametrize("kind,M,K,N", [(KIND_LIN, 64, 32768, 512), (KIND_LIN, 2, 256, 32768), (KIND_LIN, 5, 32768, 1024),
                                          (KIND_LIN, 20480, 512, 512)])   # per-tap kernel: 24 splits wanted, 23 non-empty ones launched
def test_linear_wgrad(kind, M, K, N):
    x = _rand(M, K, seed=1)
    dy = _rand(M, N, seed=2, scale=0.1)
    ref = dy.t() @ x
    got = conv_wgrad(kind, x.view(M, K, 1, 1), dy.view(M, N, 1, 1), N, (N, K))
    assert rel_err(got, ref) <= 2e-4


@pytest.mark.parametrize("B,C,HW,mode", [(2, 64, 4096, 0), (2, 64, 4096, 2), (3, 512, 64, 2), (2, 256, 256, 1), (2, 32, 16384, 0), (2, 128, 1024, 1),
                                          (1, 32, 16384, 0)])      # one sample, the most chunks per sample: P1 / P2 exactly B*nchunk*C*{2,1}
def test_gn_mish_forward_backward(B, C, HW, mode):
    _gn_mish_forward_backward(B, C, HW, mode)


def _gn_mish_forward_backward(B, C, HW, mode, skew=0):
    lib = L()
    H = int(HW ** 0.5)
    v = _rand(B, C, H, H, seed=1, scale=1.5).requires_grad_(True)
    gamma = (1 + 0.25 * _rand(C, seed=2)).requires_grad_(True)
    beta = (0.1 * _rand(C, seed=3)).requires_grad_(True)
    other = _rand(B, C, H, H, seed=4).requires_grad_(True) if mode else None
    u = F.group_norm(v, 8, gamma, beta, 1e-5)
    y = F.mish(u)
    if mode == 1:
        y = y + other
    elif mode == 2:
        y = F.mish(y + other)
    dy = _rand(B, C, H, H, seed=5)
    # partial sums as the conv epilogue would deliver them (one tile per sample)
    g5 = v.detach().double().view(B, 8, C // 8, HW)
    part = gin(torch.stack([g5.sum(dim=(2, 3)), (g5 * g5).sum(dim=(2, 3))], dim=-1).float().view(B, 1, 8, 2), skew)
    vd = _nhwc_h(v.detach(), skew)
    od = _nhwc_h(other.detach(), skew) if mode else None
    yd = guarded(tuple(vd.shape), torch.float16, "out", skew)
    stats = guarded((B, 8, 2), torch.float32, "out", skew)
    gd, bd = gin(gamma.detach(), skew), gin(beta.detach(), skew)
    lib.check(lib.lib.lo_gn_mish_forward(vd.data_ptr(), part.data_ptr(), 1, gd.data_ptr(), bd.data_ptr(), lib.ptr(od),
                                         yd.data_ptr(), stats.data_ptr(), B, HW, C, mode, lib.stream_ptr()))
    sync()
    got = from_nhwc(yd)
    assert (got - y.detach()).abs().max().item() <= 3e-3 * max(1.0, y.abs().max().item())
    # backward
    grads = torch.autograd.grad(y, [v, gamma, beta] + ([other] if mode == 2 else []), dy)
    nchunk = lib.lib.lo_gn_nchunk_for(HW, C)
    assert 0 < nchunk <= 256
    P1 = guarded(B * nchunk * C * 2, torch.float32, "out", skew)    # exactly the header's sizes
    P2 = guarded(B * nchunk * C, torch.float32, "out", skew)
    dyd = _nhwc_h(dy, skew)
    dv = guarded(tuple(vd.shape), torch.float16, "out", skew)
    ds = guarded(tuple(vd.shape), torch.float16, "out", skew) if mode == 2 else None
    dg = guarded(C, torch.float32, "out", skew)
    db = guarded(C, torch.float32, "out", skew)
    dbias = guarded(C, torch.float32, "out", skew)
    bmode = 2 if mode == 2 else 0
    lib.check(lib.lib.lo_gn_mish_backward(dyd.data_ptr(), vd.data_ptr(), lib.ptr(od) if mode == 2 else None, stats.data_ptr(),
                                          gd.data_ptr(), bd.data_ptr(), lib.ptr(ds), dv.data_ptr(), P1.data_ptr(), P2.data_ptr(),
                                          dg.data_ptr(), db.data_ptr(), dbias.data_ptr(), B, HW, C, bmode, 1.0, lib.stream_ptr()))
    sync()
    assert rel_err(from_nhwc(dv), grads[0]) <= 3e-3
    assert rel_err(dg.cpu(), grads[1]) <= 2e-3
    assert rel_err(db.cpu(), grads[2]) <= 2e-3
    assert rel_err(dbias.cpu(), grads[0].sum(dim=(0, 2, 3))) <= 5e-2 or grads[0].sum(dim=(0, 2, 3)).abs().max() < 1e-2
    if mode == 2:
        assert rel_err(from_nhwc(ds), grads[3]) <= 3e-3
    written(yd, stats, dv, ds, dg, db, dbias)
    check_guards(part, vd, od, yd, stats, gd, bd, P1, P2, dyd, dv, ds, dg, db, dbias)


@pytest.mark.parametrize("B", [1, 3])
def test_first_conv(B):
    _first_conv(B)


def _first_conv(B, skew=0, partial_short=0):
    lib = L()
    x = torch.randn(B, 3, 128, 128, generator=torch.Generator().manual_seed(1))
    w = (torch.randn(64, 3, 3, 3, generator=torch.Generator().manual_seed(2)) / 27 ** 0.5).requires_grad_(True)
    b = torch.randn(64, generator=torch.Generator().manual_seed(3)) * 0.1
    ref = F.conv2d(x, w, b, stride=2, padding=1)
    v = guarded((B, 64, 64, 64), torch.float16, "out", skew)
    part = guarded((B, 64, 8, 2), torch.float32, "out", skew)
    xd, wdev, bdev = gin(x, skew), gin(w.detach(), skew), gin(b, skew)   # keep device copies alive until the kernels have run
    lib.check(lib.lib.lo_first_conv_forward(xd.data_ptr(), wdev.data_ptr(), bdev.data_ptr(), v.data_ptr(),
                                            part.data_ptr(), B, lib.stream_ptr()))
    sync()
    got = from_nhwc(v)
    assert (got - ref.detach()).abs().max().item() <= 3e-3 * max(1.0, ref.abs().max().item())
    g5 = got.double().view(B, 8, 8, -1)
    tot = part.double().sum(dim=1).cpu()
    assert torch.allclose(tot[:, :, 0], g5.sum(dim=(2, 3)), rtol=1e-4, atol=1e-2)
    assert torch.allclose(tot[:, :, 1], (g5 * g5).sum(dim=(2, 3)), rtol=1e-4, atol=1e-2)
    dy = _rand(B, 64, 64, 64, seed=4, scale=0.1)
    (dw_ref,) = torch.autograd.grad(ref, w, dy)
    partial = guarded(B * 16 * 1728 - partial_short, torch.float32, "out", skew)   # the header's size
    dw = guarded((64, 3, 3, 3), torch.float32, "out", skew)
    dyd = _nhwc_h(dy, skew)
    lib.check(lib.lib.lo_first_conv_wgrad_op(xd.data_ptr(), dyd.data_ptr(), partial.data_ptr(), dw.data_ptr(), B, 1.0,
                                             lib.stream_ptr()))
    sync()
    assert rel_err(dw.cpu(), dw_ref) <= 1e-4
    written(v, part, dw)
    check_guards(v, part, xd, wdev, bdev, partial, dw, dyd)


@pytest.mark.parametrize("B,explicit", [(1, False), (2, True), (3, False)])
def test_final_conv(B, explicit):
    _final_conv(B, explicit)


def _final_conv(B, explicit, skew=0):
    lib = L()
    a4 = _rand(B, 32, 128, 128, seed=1).requires_grad_(True)
    w = (torch.randn(3, 32, 3, 3, generator=torch.Generator().manual_seed(2)) / 288 ** 0.5).requires_grad_(True)
    b = (torch.randn(3, generator=torch.Generator().manual_seed(3)) * 0.1).requires_grad_(True)
    target = torch.rand(B, 3, 128, 128, generator=torch.Generator().manual_seed(4)) * 2 - 1
    recon_ref = torch.tanh(F.conv2d(a4, w, b, padding=1))
    a4d = _nhwc_h(a4.detach(), skew)
    wd, bd, td = gin(w.detach(), skew), gin(b.detach(), skew), gin(target, skew)
    recon = guarded((B, 3, 128, 128), torch.float32, "out", skew)
    msep = guarded(B * 64, torch.float32, "out", skew)
    lib.check(lib.lib.lo_final_conv_forward(a4d.data_ptr(), wd.data_ptr(), bd.data_ptr(), td.data_ptr(), recon.data_ptr(),
                                            msep.data_ptr(), B, lib.stream_ptr()))
    sync()
    assert (recon.cpu() - recon_ref.detach()).abs().max().item() <= 2e-5
    mse_ref = F.mse_loss(recon_ref, target)
    assert abs(msep.double().sum().item() / target.numel() - mse_ref.item()) <= 1e-6
    scale = 1024.0
    if explicit:
        drecon = torch.randn(B, 3, 128, 128, generator=torch.Generator().manual_seed(5)) * 1e-3
        grads = torch.autograd.grad(recon_ref, [a4, w, b], drecon)
        coef = None
        dr = gin(drecon, skew)
    else:
        c = 0.37 * 2.0 / target.numel()
        grads = torch.autograd.grad(0.37 * mse_ref, [a4, w, b])
        coef = gin(torch.tensor([c * scale], dtype=torch.float32), skew)
        dr = None
    da4 = guarded(tuple(a4d.shape), torch.float16, "out", skew)
    partial = guarded(B * 64 * 867, torch.float32, "out", skew)       # the header's size
    dw = guarded((3, 32, 3, 3), torch.float32, "out", skew)
    db = guarded(3, torch.float32, "out", skew)
    lib.check(lib.lib.lo_final_conv_backward(a4d.data_ptr(), wd.data_ptr(), recon.data_ptr(), None if explicit else td.data_ptr(),
                                             lib.ptr(dr), lib.ptr(coef), scale, da4.data_ptr(), partial.data_ptr(), dw.data_ptr(),
                                             db.data_ptr(), B, 1.0 / scale, lib.stream_ptr()))
    sync()
    assert rel_err(from_nhwc(da4) / scale, grads[0]) <= 2e-3
    assert rel_err(dw.cpu(), grads[1]) <= 1e-4
    assert rel_err(db.cpu(), grads[2]) <= 1e-4
    # per pixel, where a stale patch or a non-zero border would sit: the two outermost rings of the image and the pixels either side
    # of every 16-pixel tile seam, each element against the same 2e-3 of the fp32 reference's value range (fp16 storage of da4 alone
    # is 2^-11 = 4.9e-4 of an element's own magnitude).  One wrong pixel fails here; in the L2 norm above it is 1e-5 of the sum.
    got = from_nhwc(da4) / scale
    ref = grads[0]
    idx = torch.arange(128)
    edge = (idx < 2) | (idx >= 126) | (idx % 16 == 15) | (idx % 16 == 0)
    mask = (edge.view(128, 1) | edge.view(1, 128)).view(1, 1, 128, 128).expand_as(ref)
    worst = (got - ref).abs()[mask].max().item()
    print("final conv B=%d: da4 worst border / seam pixel error %.3e of range %.3e" % (B, worst, ref.abs().max().item()))
    assert worst <= 2e-3 * ref.abs().max().item(), (worst, ref.abs().max().item())
    written(recon, msep, da4, dw, db)
    check_guards(a4d, wd, bd, td, recon, msep, dr, coef, da4, partial, dw, db)


def test_clip_adamw_matches_torch():
    _clip_adamw_matches_torch()


def _clip_adamw_matches_torch(skew=0):
    lib = L()
    n = 1_000_003
    g = torch.Generator().manual_seed(0)
    p = torch.randn(n, generator=g)
    p_ref = p.clone().requires_grad_(True)
    opt = torch.optim.AdamW([p_ref], lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999))
    pd, md, vd = gin(p, skew), gin(torch.zeros(n), skew), gin(torch.zeros(n), skew)     # n = 1_000_003 ends off every vector boundary
    scratch = gin(torch.zeros(1028, dtype=torch.float32), skew)
    for step in range(1, 4):
        grad = torch.randn(n, generator=g) * 0.01 * step
        p_ref.grad = grad.clone()
        norm = torch.nn.utils.clip_grad_norm_([p_ref], 1.0)
        opt.step()
        gd = gin(grad, skew)
        lib.check(lib.lib.lo_clip_adamw_step(pd.data_ptr(), gd.data_ptr(), md.data_ptr(), vd.data_ptr(), n, 1.0, 1e-3, 0.9, 0.999,
                                             1e-8, 0.01, step, scratch.data_ptr(), lib.stream_ptr()))
        sync()
        assert abs(scratch[1024].item() - norm.item()) <= 1e-4 * norm.item()
        assert (pd.cpu() - p_ref.detach()).abs().max().item() <= 2e-6
        check_guards(pd, gd, md, vd, scratch)


@pytest.mark.parametrize("B,C,H", [(2, 64, 8), (2, 128, 16), (1, 512, 8)])
def test_selfattention2d_forward_backward(B, C, H):
    """Fused attention vs the oracle restatement (and vs the golden fixture generated from the reference module); the
    backward vs autograd of the oracle."""
    _selfattention2d_forward_backward(B, C, H)


def _selfattention2d_forward_backward(B, C, H, skew=0):
    import os

    import numpy as np

    from lunaris_orion_amd.vae import SelfAttention2d
    from oracle import vae_ref as R
    m = SelfAttention2d(C)
    sd = {}
    for k, v in m.state_dict().items():
        t = R.closed_form_tensor("attn." + k, tuple(v.shape))
        sd[k] = t if v.dim() > 1 else t * 0 + 0.05
    sd["gamma"] = torch.tensor([0.7])
    m.load_state_dict(sd)
    x = R.closed_form_tensor("attn.x", (B, C, H, H)) * 8.0
    ref = R.self_attention_2d(x, sd["query_conv.weight"], sd["query_conv.bias"], sd["key_conv.weight"], sd["key_conv.bias"],
                              sd["value_conv.weight"], sd["value_conv.bias"], sd["gamma"])
    with torch.no_grad():
        got = m.cuda()(x.cuda()).cpu()
    # forward: the 1x1 projections run on the exact fp32 matrix instruction, QK^T and PV on fp16 MFMA operands with fp32
    # accumulation and an online fp32 softmax -> stated tolerance 4e-3 of the output range (fp16 keeps 11 significant bits;
    # measured <= 1.5e-3).  The fp32 VALU kernels (LO_ATTN_FP32=1, 2e-5) are checked in a subprocess below.
    err = (got - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    print("selfattn2d", (B, C, H), "forward error / range", err)
    assert err <= 4e-3, err
    if (B, C, H) == (2, 64, 8):
        g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "selfattn2d.npz"))
        assert np.abs(got.numpy() - g["y"]).max() <= 4e-3 * max(1.0, np.abs(g["y"]).max())
    # backward: every gradient against autograd of the oracle restatement (fp32 both sides)
    xr = x.clone().requires_grad_(True)
    Pr = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    yr = R.self_attention_2d(xr, Pr["query_conv.weight"], Pr["query_conv.bias"], Pr["key_conv.weight"], Pr["key_conv.bias"],
                             Pr["value_conv.weight"], Pr["value_conv.bias"], Pr["gamma"])
    dy = R.closed_form_tensor("attn.dy", tuple(yr.shape))
    yr.backward(dy)
    xg = x.cuda().requires_grad_(True)
    m.zero_grad()
    m(xg).backward(dy.cuda())
    got_g = {"x": xg.grad.cpu(), **{k: p.grad.cpu() for k, p in m.named_parameters()}}
    ref_g = {"x": xr.grad, **{k: Pr[k].grad for k in Pr}}
    for k in ref_g:
        scale = max(1e-3, ref_g[k].abs().max().item())
        assert (got_g[k] - ref_g[k]).abs().max().item() <= 2e-4 * scale + 1e-6, (k, (got_g[k] - ref_g[k]).abs().max().item(), scale)
    _selfattention2d_c_abi_guarded(B, C, H, sd, x, dy, ref, ref_g, skew)


def _selfattention2d_c_abi_guarded(B, C, H, sd, x, dy, ref, ref_g, skew=0):
    """The same two calls as the module makes (lo_selfattn2d_forward / _backward), on guard-banded buffers of the header's sizes:
    the same references and tolerances as above, and every guard intact."""
    lib = L()
    N = H * H
    st = lib.stream_ptr()
    xd = gin(x.view(B, C, N), skew)
    names = ("query_conv.weight", "query_conv.bias", "key_conv.weight", "key_conv.bias", "value_conv.weight", "value_conv.bias", "gamma")
    P = [gin(sd[k], skew) for k in names]
    q = guarded((B, C // 8, N), torch.float32, "out", skew)
    k_ = guarded((B, C // 8, N), torch.float32, "out", skew)
    v = guarded((B, C, N), torch.float32, "out", skew)
    out = guarded((B, C, N), torch.float32, "out", skew)
    lib.check(lib.lib.lo_selfattn2d_forward(xd.data_ptr(), *[t.data_ptr() for t in P], q.data_ptr(), k_.data_ptr(), v.data_ptr(),
                                            out.data_ptr(), B, C, N, st), "lo_selfattn2d_forward")
    sync()
    err = (out.cpu().view_as(ref) - ref).abs().max().item() / max(1.0, ref.abs().max().item())
    assert err <= 4e-3, err
    dyd = gin(dy.view(B, C, N), skew)
    scratch = guarded(lib.lib.lo_selfattn2d_backward_scratch_elems(B, C, N), torch.float32, "out", skew)
    dx = guarded((B, C, N), torch.float32, "out", skew)
    dwq, dwk, dwv = (guarded(tuple(sd[n].shape), torch.float32, "out", skew) for n in names[0:6:2])
    dbq, dbk, dbv = (guarded(tuple(sd[n].shape), torch.float32, "out", skew) for n in names[1:6:2])
    dg = guarded(1, torch.float32, "out", skew)
    lib.check(lib.lib.lo_selfattn2d_backward(xd.data_ptr(), P[0].data_ptr(), P[2].data_ptr(), P[4].data_ptr(), P[6].data_ptr(), q.data_ptr(),
                                             k_.data_ptr(), v.data_ptr(), dyd.data_ptr(), scratch.data_ptr(), dx.data_ptr(),
                                             dwq.data_ptr(), dbq.data_ptr(), dwk.data_ptr(), dbk.data_ptr(), dwv.data_ptr(),
                                             dbv.data_ptr(), dg.data_ptr(), B, C, N, st), "lo_selfattn2d_backward")
    sync()
    got_g = {"x": dx.cpu().view_as(ref), "query_conv.weight": dwq.cpu(), "query_conv.bias": dbq.cpu(), "key_conv.weight": dwk.cpu(),
             "key_conv.bias": dbk.cpu(), "value_conv.weight": dwv.cpu(), "value_conv.bias": dbv.cpu(), "gamma": dg.cpu()}
    for k in ref_g:
        scale = max(1e-3, ref_g[k].abs().max().item())
        assert (got_g[k] - ref_g[k]).abs().max().item() <= 2e-4 * scale + 1e-6, (k, (got_g[k] - ref_g[k]).abs().max().item(), scale)
    written(q, k_, v, out, dx, dwq, dwk, dwv, dbq, dbk, dbv, dg)
    check_guards(xd, *P, q, k_, v, out, dyd, scratch, dx, dwq, dwk, dwv, dbq, dbk, dbv, dg)


def test_selfattention2d_fp32_kernels_strict_parity():
    """LO_ATTN_FP32=1: the two-pass fp32 VALU kernels (first-round form) keep the 2e-5 module-level parity; the knob is read
    once per process, hence the subprocess."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r"""
import sys, torch
sys.path.insert(0, %r)
from oracle import vae_ref as R
from lunaris_orion_amd.vae import SelfAttention2d
C, B, H = 128, 2, 16
m = SelfAttention2d(C)
sd = {k: (R.closed_form_tensor("attn." + k, tuple(v.shape)) if v.dim() > 1 else R.closed_form_tensor("attn." + k, tuple(v.shape)) * 0 + 0.05) for k, v in m.state_dict().items()}
sd["gamma"] = torch.tensor([0.7]); m.load_state_dict(sd)
x = R.closed_form_tensor("attn.x", (B, C, H, H)) * 8.0
ref = R.self_attention_2d(x, sd["query_conv.weight"], sd["query_conv.bias"], sd["key_conv.weight"], sd["key_conv.bias"], sd["value_conv.weight"], sd["value_conv.bias"], sd["gamma"])
with torch.no_grad():
    got = m.cuda()(x.cuda()).cpu()
assert (got - ref).abs().max().item() <= 2e-5 * max(1.0, ref.abs().max().item())
print("ATTN_FP32_OK")
""" % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=dict(os.environ, LO_ATTN_FP32="1"))
    assert "ATTN_FP32_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]


@pytest.mark.parametrize("world,fp16_wire", [(2, True), (4, True), (8, True), (8, False), (3, True)])
def test_direct_exchange_arithmetic_of_n_ranks_on_one_device(world, fp16_wire):
    """The data-parallel exchange of lunaris_orion_amd/parallel.py (`mode="direct"`) for `world` ranks, with the two collectives
    replaced by the copies they perform (all_to_all_single: recv_r[j] = body_j[chunk r]; all_gather_into_tensor: body[j] = share_j),
    so the library kernels (lo_dp_pack_f16 / lo_dp_sum_shares / lo_dp_unpack_f16) see exactly the buffers an N-rank RCCL group
    would hand them.  Result on every rank == the mean of the ranks' gradients: to fp32 rounding on the fp32 wire, to the fp16
    wire's resolution (values * 1024 in fp16: 2^-11 relative per element, twice) on the fp16 wire."""
    _direct_exchange(world, fp16_wire)


def _direct_exchange(world, fp16_wire, skew=0):
    from lunaris_orion_amd import _lib
    lib = L()
    n = 1000 * world + 37 * world          # divisible by world (the remainder goes through a plain all-reduce in parallel.py)
    g = torch.Generator().manual_seed(5)
    grads = [gin(torch.randn(n, generator=g) * 10.0 ** torch.randint(-6, -2, (n,), generator=g).float(), skew) for _ in range(world)]
    ref = torch.stack([t.double() for t in grads]).mean(0)
    st = _lib.stream_ptr()
    chunk = n // world
    if fp16_wire:
        bodies = [guarded(n, torch.float16, "out", skew) for _ in range(world)]
        for t, w in zip(grads, bodies):
            _lib.check(lib.lib.lo_dp_pack_f16(t.data_ptr(), w.data_ptr(), n, 1024.0, st), "pack")
    else:
        bodies = [gin(t, skew) for t in grads]
    shares = []
    for r in range(world):                                          # rank r's side of the all-to-all + its share sum
        recv = gin(torch.cat([bodies[j][r * chunk:(r + 1) * chunk] for j in range(world)]), skew)
        share = guarded(chunk, recv.dtype, "out", skew)
        _lib.check(lib.lib.lo_dp_sum_shares(recv.data_ptr(), share.data_ptr(), world, chunk, 1 if fp16_wire else 0, st), "sum")
        shares.append(share)
        sync()
        check_guards(recv, share)
    gathered = gin(torch.cat(shares), skew)                                # what all_gather_into_tensor leaves in every rank's body
    out = guarded(n, torch.float32, "out", skew)
    if fp16_wire:
        _lib.check(lib.lib.lo_dp_unpack_f16(gathered.data_ptr(), out.data_ptr(), n, 1.0 / 1024.0, st), "unpack")
        # the fused form (unpack + the early part of the gradient norm in one pass): same values bit for bit, and scratch[512..1024)
        # holds the partial sums of squares lo_gradnorm_early_range would leave there
        out2 = guarded(n, torch.float32, "out", skew)
        scratch = gin(torch.zeros(1028, dtype=torch.float32), skew)
        scratch2 = gin(torch.zeros(1028, dtype=torch.float32), skew)
        _lib.check(lib.lib.lo_dp_unpack_f16_sumsq(gathered.data_ptr(), out2.data_ptr(), n, 1.0 / 1024.0, scratch.data_ptr(), st), "unpack_sumsq")
        _lib.check(lib.lib.lo_gradnorm_early_range(out.data_ptr(), 0, n, scratch2.data_ptr(), st), "early_range")
        sync()
        assert torch.equal(out, out2)
        ss = out.double().pow(2).sum().item()
        assert abs(scratch[512:1024].double().sum().item() - ss) <= 1e-6 * ss and abs(scratch2[512:1024].double().sum().item() - ss) <= 1e-6 * ss
        assert scratch[:512].abs().sum().item() == 0 and scratch[1024:].abs().sum().item() == 0
        check_guards(out2, scratch, scratch2)
    else:
        out.copy_(gathered)
    sync()
    written(out)
    check_guards(*grads, *bodies, gathered, out)
    err = (out.double().cpu() - ref.cpu()).abs()
    scale = torch.stack([t.abs().double() for t in grads]).max(0).values.cpu()
    if fp16_wire:
        # fp16 normal range after the x1024 scale starts at 6e-8 / 1024: smaller elements lose relative precision, bound absolutely
        assert (err <= 1.5e-3 * scale + 1e-10).all(), (err / (scale + 1e-30)).max().item()
    else:
        assert (err <= 1e-6 * scale + 1e-30).all(), (err / (scale + 1e-30)).max().item()


# ---- one case of each op at exactly the promised alignment: every pointer at (a multiple of 256 B) + 16 B --------------------------
def test_conv_forward_and_gn_partials_aligned16():
    _conv_forward_and_gn_partials(KIND_S1, 2, 128, 128, 32, skew=16)
    _conv_forward_and_gn_partials(KIND_S2, 2, 64, 128, 64, skew=16)
    _conv_forward_and_gn_partials(KIND_T4, 2, 64, 32, 64, skew=16)


def test_conv_dgrad_aligned16():
    _conv_dgrad(KIND_S1D, KIND_S1, 2, 64, 64, 64, skew=16)
    _conv_dgrad(KIND_S2D, KIND_S2, 2, 256, 512, 16, skew=16)
    _conv_dgrad(KIND_T4D, KIND_T4, 2, 512, 256, 8, skew=16)


def test_conv_wgrad_aligned16():
    _conv_wgrad(KIND_S1, 3, 256, 256, 16, skew=16)
    _conv_wgrad(KIND_S2, 1, 64, 128, 16, skew=16)
    _conv_wgrad(KIND_T4, 1, 64, 32, 8, skew=16)


def test_linear_splitk_aligned16():
    _linear_splitk(37, 1024, 64, 3, skew=16)


def test_gn_mish_forward_backward_aligned16():
    _gn_mish_forward_backward(3, 512, 64, 2, skew=16)


def test_selfattention2d_forward_backward_aligned16():
    _selfattention2d_forward_backward(2, 128, 16, skew=16)


def test_first_conv_aligned16():
    _first_conv(2, skew=16)


def test_final_conv_aligned16():
    _final_conv(1, False, skew=16)


def test_clip_adamw_matches_torch_aligned16():
    _clip_adamw_matches_torch(skew=16)


def test_direct_exchange_arithmetic_aligned16():
    _direct_exchange(3, True, skew=16)
    _direct_exchange(2, False, skew=16)


# ---- the guards bite: one slab / one partial row fewer than the ABI's size (the stray write stays inside the guard band) ----------
def test_check_guards_names_a_linear_slab_one_split_short():
    with pytest.raises(AssertionError, match=r"guard band ABOVE argument 2 .* a write beyond the tensor"):
        _linear_splitk(37, 1024, 64, 3, slab_short=1)


def test_check_guards_names_a_first_conv_partial_table_one_row_short():
    with pytest.raises(AssertionError, match=r"guard band ABOVE argument 5 .* a write beyond the tensor"):
        _first_conv(2, partial_short=1728)
