#!/usr/bin/env python
"""Micro-benchmark of one implicit-GEMM op through the C ABI (tuning aid; also the target of rocprofv3 --pmc runs).

  python tools/op_bench.py --op conv|wgrad --kind 0 --B 64 --H 32 --Cin 128 --Cout 128 --iters 20
  python tools/op_bench.py --op attn --B 64 --H 8 --Cin 512        (SelfAttention2d forward on a [B, Cin, H, H] map)
  python tools/op_bench.py --op imgdgrad --stride 2|1 --B 64       (images' data gradient: VAE encoder.down1.0 | teacher conv1)
  python tools/op_bench.py --op tconv --B 8 --pairs 3              (wide teacher 3x3 convs at 128x128, e4m3 against fp16, interleaved; markdown table)
  python tools/op_bench.py --op lowrank_gathered --B 64 --pairs 3  (data parallel: norm + AdamW of the two Linear matrices from gathered factors, mode 3 against mode 2, world 1 / 2 / 4 / 8)
"""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lunaris_orion_amd import _lib  # noqa: E402


def tconv(a):
    """The feature_dim 256 / 512 teacher's 3x3 convolutions at 128x128: the e4m3 launch (lo_teacher_conv3x3_forward_f8: LeakyReLU + BatchNorm
    partial rows) against the fp16 launch of the same shape (lo_conv_forward kind 0 with its partial sums), `--pairs` interleaved pairs of
    `--iters` launches each after a warm-up of both.  Prints one markdown table row per shape: the best and the worst of the pairs."""
    lib, st, B, H = _lib.lib, _lib.stream_ptr(), a.B, 128
    print(f"| shape (B = {B}, 128x128) | fp16 us (pairs) | e4m3 us (pairs) | fp16 TFLOP/s (of 2500) | e4m3 TFLOP/s (of 5000) | e4m3 faster in every pair |")
    print("|---|---|---|---|---|---|")
    for Cin, Cout in ((128, 256), (256, 256), (128, 512), (512, 512)):
        x = torch.nn.functional.leaky_relu(torch.randn(B, H, H, Cin, device="cuda"), 0.2).half()
        n = lib.lo_packed_weight_elems_for(0, B, H, H, Cin, Cout)
        wp = (torch.randn(n, device="cuda") * (9 * Cin) ** -0.5).half()
        bias = torch.randn(Cout, device="cuda") * 0.1
        x8, w8 = torch.empty(x.numel(), dtype=torch.uint8, device="cuda"), torch.empty(n, dtype=torch.uint8, device="cuda")
        ws = torch.empty(Cout, device="cuda")
        _lib.check(lib.lo_quantize_act_f8(x.data_ptr(), x8.data_ptr(), x.numel(), st))
        _lib.check(lib.lo_pack_weight_f8_for(0, B, H, H, Cin, Cout, wp.data_ptr(), w8.data_ptr(), ws.data_ptr(), st))
        out = torch.empty(B, H, H, Cout, dtype=torch.float16, device="cuda")
        part = torch.empty(B * H * H // 64 * Cout * 2, device="cuda")
        mt, rows = C.c_int(0), C.c_int(0)
        fl = 2.0 * B * H * H * Cout * 9 * Cin

        def run16():
            _lib.check(lib.lo_conv_forward(0, B, H, H, Cin, Cout, x.data_ptr(), wp.data_ptr(), bias.data_ptr(), None, out.data_ptr(), part.data_ptr(), C.byref(mt), st))

        def run8():
            _lib.check(lib.lo_teacher_conv3x3_forward_f8(B, H, H, Cin, Cout, x8.data_ptr(), w8.data_ptr(), ws.data_ptr(), bias.data_ptr(), 1, out.data_ptr(),
                                                         part.data_ptr(), C.byref(rows), st))

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.iters * 1e3
        for fn in (run16, run8):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        t16, t8 = [], []
        for _ in range(a.pairs):
            t16.append(timed(run16))
            t8.append(timed(run8))
        tf = lambda us: fl / us / 1e6
        print(f"| {Cin} -> {Cout} | {' / '.join(f'{t:.1f}' for t in t16)} | {' / '.join(f'{t:.1f}' for t in t8)} | "
              f"{tf(max(t16)):.0f}-{tf(min(t16)):.0f} ({tf(min(t16)) / 2500:.2f}) | {tf(max(t8)):.0f}-{tf(min(t8)):.0f} ({tf(min(t8)) / 5000:.2f}) | "
              f"{'yes' if all(p8 < p16 for p8, p16 in zip(t8, t16)) else 'NO'} |", flush=True)


def lowrank_gathered(a):
    """Data parallel, the two Linear weight matrices at batch `--B` / latent 512 from `world` synthetic gathered factor blocks on one GPU:
    mode 3 (Gram norm + factored AdamW straight from the blocks) against the passes mode 2 runs for the same result (materialise the
    averaged matrices, sum their squares, AdamW with the fp16 copy, the two transposes), each matrix by its own launches on both sides
    (the step puts both matrices of mode 3 into one launch per pass).  Two buffer sets alternate; one call moves 1.2 - 2 GB, several
    times the 256 MB last-level cache, so every call streams from HBM.  `--pairs` interleaved pairs of `--iters` calls; markdown rows."""
    lib, st, B, L = _lib.lib, _lib.stream_ptr(), a.B, 512
    Bp = (B + 31) // 32 * 32
    h = C.c_void_p()
    _lib.check(lib.lo_vae_create(B, L, C.byref(h)))
    fo, fb, pb, pe, lb, le = (C.c_size_t() for _ in range(6))
    _lib.check(lib.lo_vae_factor_block(h, C.byref(fo), C.byref(fb)))
    _lib.check(lib.lo_vae_phase1_grad_range(h, C.byref(pb), C.byref(pe)))
    _lib.check(lib.lo_vae_linear_grad_range(h, C.byref(lb), C.byref(le)))
    o_dml, o_x = 0, 2 * L * Bp
    o_gfc = o_x + 32768 * Bp
    o_z = o_gfc + 32768 * Bp
    blk = o_z + L * Bp                                   # elements per rank block: dml^T | xflat^T | Gfc^T | z^T
    assert blk * 2 == fb.value, (blk * 2, fb.value)
    nflat = lib.lo_vae_flat_elems(h)
    bh, nh = pb.value, 2 * L * 32768
    bd, nd = le.value - 32768 - 32768 * L, 32768 * L
    mats = ((bh, 2 * L, 32768, o_x, o_dml), (bd, 32768, L, o_z, o_gfc))       # offset, N, K, xt, yt
    hyp = (1e-4, 0.9, 0.999, 1e-8, 0.01, 3)
    print(f"| world | K = world x Bp | mode 3: norm us | mode 3: AdamW us | mode 3 total us (pairs) | mode 2: materialise us | mode 2: norm us | mode 2: AdamW + cast us | "
          f"mode 2: transposes us | mode 2 total us (pairs) | mode 2 / mode 3 |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    sets = []
    for _ in range(2):
        P = torch.randn(nflat, device="cuda") * 0.02
        sets.append(dict(P=P, M=torch.zeros_like(P), V=torch.zeros_like(P), G=torch.empty_like(P), c=[torch.empty(nh, dtype=torch.float16, device="cuda"),
                    torch.empty(nd, dtype=torch.float16, device="cuda")], ct=[torch.empty(nh, dtype=torch.float16, device="cuda"),
                    torch.empty(nd, dtype=torch.float16, device="cuda")], scratch=torch.zeros(1028, device="cuda")))
    norm = torch.tensor([1.0, 1.0, 1.0], device="cuda")
    for world in (1, 2, 4, 8):
        gram = torch.empty(lib.lo_vae_gathered_scratch_bytes(h, world) // 4, device="cuda")
        gath = []
        for _ in range(2):
            g = torch.zeros(world, blk, dtype=torch.float16, device="cuda")
            for off, rows in ((o_dml, 2 * L), (o_x, 32768), (o_gfc, 32768), (o_z, L)):
                g[:, off:off + rows * Bp].view(world, rows, Bp)[:, :, :B] = (torch.randn(world, rows, B, device="cuda") * 0.05).half()
            gath.append(g)
        kt = world * Bp
        it = [0]

        def new_norm():
            s, g = sets[it[0] % 2], gath[it[0] % 2]
            for i, (off, N, K, xo, yo) in enumerate(mats):
                short, ns, long_, nl = (yo, N, xo, K) if N < K else (xo, K, yo, N)
                _lib.check(lib.lo_lowrank_gathered_sumsq(g.data_ptr() + 2 * short, ns, g.data_ptr() + 2 * long_, nl, blk, world, B, 1.0 / world,
                                                         gram.data_ptr() + 4 * i * kt * kt, s["scratch"].data_ptr() + 4 * (768 + 128 * i), st))

        def new_adamw():
            s, g = sets[it[0] % 2], gath[it[0] % 2]
            for i, (off, N, K, xo, yo) in enumerate(mats):
                _lib.check(lib.lo_lowrank_gathered_adamw(s["P"].data_ptr() + 4 * off, s["M"].data_ptr() + 4 * off, s["V"].data_ptr() + 4 * off, s["c"][i].data_ptr(),
                                                         s["ct"][i].data_ptr(), g.data_ptr() + 2 * xo, g.data_ptr() + 2 * yo, blk, world, N, K, B, 1.0 / world,
                                                         norm.data_ptr(), *hyp, st))

        def old_mat():
            s, g = sets[it[0] % 2], gath[it[0] % 2]
            _lib.check(lib.lo_vae_materialize_gathered_linear_grads(h, g.data_ptr(), world, s["G"].data_ptr(), st))

        def old_norm():
            s = sets[it[0] % 2]
            for off, N, K, _, _ in mats:
                _lib.check(lib.lo_gradnorm_early_range(s["G"].data_ptr(), off, off + N * K, s["scratch"].data_ptr(), st))

        def old_adamw():
            s = sets[it[0] % 2]
            for i, (off, N, K, _, _) in enumerate(mats):
                _lib.check(lib.lo_adamw_range(s["P"].data_ptr() + 4 * off, s["G"].data_ptr() + 4 * off, s["M"].data_ptr() + 4 * off, s["V"].data_ptr() + 4 * off,
                                              N * K, norm.data_ptr(), *hyp, s["c"][i].data_ptr(), st))

        def old_tr():
            s = sets[it[0] % 2]
            for i, (off, N, K, _, _) in enumerate(mats):
                _lib.check(lib.lo_transpose_f16(s["c"][i].data_ptr(), s["ct"][i].data_ptr(), N, K, st))

        def timed(parts):
            """mean us per call of each part and of their sum, the parts of one call back to back in stream order"""
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(len(parts) + 1)] for _ in range(a.iters)]
            for k in range(a.iters):
                ev[k][0].record()
                for j, fn in enumerate(parts):
                    fn()
                    ev[k][j + 1].record()
                it[0] += 1
            torch.cuda.synchronize()
            per = [sum(e[j].elapsed_time(e[j + 1]) for e in ev) / a.iters * 1e3 for j in range(len(parts))]
            return per, sum(e[0].elapsed_time(e[-1]) for e in ev) / a.iters * 1e3
        new, old = (new_norm, new_adamw), (old_mat, old_norm, old_adamw, old_tr)
        for _ in range(3):
            timed(new)
            timed(old)
        tn, to = [], []
        for _ in range(a.pairs):
            tn.append(timed(new))
            to.append(timed(old))
        bn, bo = min(tn, key=lambda t: t[1]), min(to, key=lambda t: t[1])
        print(f"| {world} | {kt} | {bn[0][0]:.0f} | {bn[0][1]:.0f} | {' / '.join(f'{t[1]:.0f}' for t in tn)} | {bo[0][0]:.0f} | {bo[0][1]:.0f} | {bo[0][2]:.0f} | {bo[0][3]:.0f} | "
              f"{' / '.join(f'{t[1]:.0f}' for t in to)} | {min(t[1] for t in to) / min(t[1] for t in tn):.2f} |", flush=True)
    lib.lo_vae_destroy(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--op", default="conv")
    ap.add_argument("--kind", type=int, default=0)
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--H", type=int, default=32)
    ap.add_argument("--Cin", type=int, default=128)
    ap.add_argument("--Cout", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--stats", type=int, default=1)
    ap.add_argument("--stride", type=int, default=2, help="--op imgdgrad: 2 = the VAE's first conv (64 channels), 1 = the teacher's conv1 (32)")
    ap.add_argument("--pairs", type=int, default=3, help="--op tconv / lowrank_gathered: interleaved pairs per shape")
    a = ap.parse_args()
    if a.op == "tconv":
        return tconv(a)
    if a.op == "lowrank_gathered":
        return lowrank_gathered(a)
    lib = _lib.lib
    B, H, Cin, Cout, kind = a.B, a.H, a.Cin, a.Cout, a.kind
    Ho = H if kind in (0, 3, 6) else (H // 2 if kind in (1, 5) else 2 * H)
    st = _lib.stream_ptr()
    if a.op == "attn":
        # SelfAttention2d forward (lunar_generate.py:56-78): roofline line of the fused kernel.  FLOPs = QK^T + PV (the three
        # 1x1 projections are separate launches and are timed with it; their FLOPs are counted too)
        Cc, N, D = Cin, H * H, Cin // 8
        xa = torch.randn(B, Cc, N, device="cuda")
        ws = [torch.randn(D, Cc, device="cuda") * Cc ** -0.5, torch.zeros(D, device="cuda"), torch.randn(D, Cc, device="cuda") * Cc ** -0.5,
              torch.zeros(D, device="cuda"), torch.randn(Cc, Cc, device="cuda") * Cc ** -0.5, torch.zeros(Cc, device="cuda"), torch.full((1,), 0.7, device="cuda")]
        q, k = torch.empty(B, D, N, device="cuda"), torch.empty(B, D, N, device="cuda")
        v, out = torch.empty(B, Cc, N, device="cuda"), torch.empty(B, Cc, N, device="cuda")
        fl_core = 2.0 * B * N * N * (D + Cc)
        fl_proj = 2.0 * B * N * Cc * (2 * D + Cc)

        def run_attn():
            _lib.check(lib.lo_selfattn2d_forward(xa.data_ptr(), *[t.data_ptr() for t in ws], q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, Cc, N, st))
        for _ in range(3):
            run_attn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            run_attn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        byts = 4.0 * B * N * (2.0 * D + 3.0 * Cc)
        print(f"attn B={B} C={Cc} N={N}: {ms * 1e3:.1f} us/call (one q|k|v projection launch + fused attention)  {(fl_core + fl_proj) / ms / 1e9:.2f} TFLOP/s "
              f"= {(fl_core + fl_proj) / ms / 1e9 / 2500.0:.4f} of the dense fp16 MFMA peak;  {byts / ms / 1e6:.1f} GB/s of q/k/v/x/out traffic = {byts / ms / 1e6 / 8000.0:.4f} of HBM peak")
        return
    if a.op == "imgdgrad":
        # lo_image_dgrad_op: dy fp16 NHWC -> dx fp32 NCHW [B,3,128,128].  Bytes = dy read once + dx written once; the calls rotate over
        # buffer sets larger than the 256 MB last-level cache together, so every call reads dy from HBM
        s_, co = a.stride, (64 if a.stride == 2 else 32)
        ho = 128 // s_
        byts = B * (ho * ho * co * 2 + 3 * 16384 * 4)
        nset = max(2, -(-320 * 2 ** 20 // byts))
        dys = [(torch.randn(B, ho, ho, co, device="cuda") * 0.1).half() for _ in range(nset)]
        dxs = [torch.empty(B, 3, 128, 128, device="cuda") for _ in range(nset)]
        w = torch.randn(co, 3, 3, 3, device="cuda") * 0.2
        fl = 2.0 * B * ho * ho * co * 27
        it = [0]

        def run():
            i = it[0] % nset
            it[0] += 1
            _lib.check(lib.lo_image_dgrad_op(dys[i].data_ptr(), co, s_, w.data_ptr(), B, 1.0, dxs[i].data_ptr(), st))
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            run()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / a.iters
        print(f"imgdgrad stride={s_} Cout={co} B={B}: {ms * 1e3:.1f} us/call  {byts / ms / 1e9:.2f} TB/s over {byts / 1e6:.1f} MB "
              f"(dy read + dx write) = {byts / ms / 1e9 / 8.0:.3f} of the 8 TB/s HBM peak;  {fl / ms / 1e9:.2f} TFLOP/s")
        return
    x = (torch.randn(B, H, H, Cin, device="cuda") * 0.5).half()
    if a.op == "conv":
        n = lib.lo_packed_weight_elems_for(kind, B, H, H, Cin, Cout)
        wp = (torch.randn(n, device="cuda") * 0.05).half()
        bias = torch.zeros(Cout, device="cuda")
        out = torch.empty(B, Ho, Ho, Cout, dtype=torch.float16, device="cuda")
        part = torch.empty(B * 4096 * 16, device="cuda") if a.stats and kind in (0, 1, 2) else None
        mt = C.c_int(0)
        fl = 2.0 * out.numel() * (n / Cout)

        def run():
            _lib.check(lib.lo_conv_forward(kind, B, H, H, Cin, Cout, x.data_ptr(), wp.data_ptr(), bias.data_ptr(), None,
                                           out.data_ptr(), _lib.ptr(part), C.byref(mt), st))
    else:
        dy = (torch.randn(B, Ho, Ho, Cout, device="cuda") * 0.1).half()
        nb = lib.lo_wgrad_slab_bytes_for(kind, B, H, H, Cin, Cout)
        slab = torch.empty(nb // 4 + 1, device="cuda")
        n = lib.lo_packed_weight_elems_for(kind, B, H, H, Cin, Cout)
        grad = torch.empty(n, device="cuda")
        fl = 2.0 * dy.numel() * (n / Cout)

        def run():
            _lib.check(lib.lo_conv_wgrad(kind, B, H, H, Cin, Cout, x.data_ptr(), dy.data_ptr(), slab.data_ptr(), grad.data_ptr(), 1.0, st))
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.iters
    print(f"{a.op} kind={kind} B={B} H={H} Cin={Cin} Cout={Cout}: {ms * 1e3:.1f} us/call  {fl / ms / 1e9:.1f} TFLOP/s")


if __name__ == "__main__":
    main()
