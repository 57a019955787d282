"""In-situ layer parity of the teacher forward: every layer against a float64 restatement of THAT operation on ITS OWN stored operands.

Every other teacher test compares head outputs (five small tensors behind a global average pool, a LayerNorm and a sigmoid) or
parameter gradients.  Here one forward runs per configuration, every tensor it leaves behind is read where lo_teacher_debug_tensor says
it lives, and each layer is checked on its own: the operands are the fp16 tensors as stored, the fp32 parameters, the weights rounded
through fp16 where the pack does, and the masks of oracle/dropout_ref.py.  A reference starts from stored operands, so it inherits no
error from upstream, and a wrong border column, channel offset, partial-row count or query token shows at the layer that has it.
The float64 restatements run in torch on the device (elementwise, reductions and matmul in float64); the masks come from numpy.

Kept forward, plain form (lo_teacher_forward_keep / _keep_eval; the 3x3 and 1x1 convs run on lo_igemm_nt with the teacher epilogue):
    K1  feature_dim 128, batch 3, train, dropout 0     odd batch, tables without masks, running statistics
    K2  feature_dim 128, batch 2, train, dropout 0.1   all six dropout sites
    K3  feature_dim 256, batch 1, train, dropout 0.1   shortcut conv + BatchNorm, id_ss in the tail, lo_t_attn_generic_kernel<32>,
                                                       lo_t_projdrop_kernel<5>, the 128 -> F and F -> F geometries
    K4  feature_dim 128, batch 2, eval                 running statistics in the tables, no state written
Production route (lo_teacher_forward, train, dropout 0.1: path 2, t_block_dropout), the tensors of block (E-1, 2) in the workspace:
    P0  batch 2, default knobs        P1  batch 2, LO_HALO=3, fresh child process        P2  batch 16        P3  batch 2, mfma_precision="fp8"
On this route t_conv3_full takes lo_conv3_run_pp_xf whenever lo_conv3_pp_applies(g3) -- which holds for the teacher's 128 x 128 x 128 -> 128
geometry at EVERY batch size and does not read LO_HALO -- so P0, P1 and P2 all run lo_conv3x3_pp<128, 16 x 16> (128 / 128 / 1024 tiles:
the short and the long grid), not lo_igemm_nt; P3 runs lo_conv3x3_pp<f8>.  Which kernel ran is asserted twice: through the profiler
names (the launch's tag says path 2 and e4m3 or not), and by running the op-level entry of the fused-tap kernel
(lo_conv3x3_fused_tap_forward) on the stored input: it must reproduce the stored o_rawA bit for bit.  lo_igemm_nt with the teacher
epilogue is what K1-K4 run.

3x3, depthwise and first convs are checked on image rows 0-7, 60-67, 120-127 (both borders and the interior, every column, every
sample); 1x1 convs, statistics, elementwise layers and pools on the whole tensor.

Bounds (none is taken from the code under test):
  round-once kernels (first conv, depthwise, BatchNorm apply / tail, catd, attention, proj_drop rows 0-7): fp32 accumulation of n
      products and ONE rounding to fp16: |got - ref| <= 2^-10 |ref| + 2^-24 (one fp16 ulp at the reference's magnitude; 2^-24 = the
      subnormal spacing) + n 2^-24 sum|terms| (n roundings of at most 2^-24 relative each on partial sums bounded by sum|terms|).
      n = 28 first conv (27 products + bias), K^2 + 1 depthwise, 8 for the apply / tail / catd (a (scale, shift) table built in fp32
      from (mean, rstd): 3 roundings per entry, then one fma each for BatchNorm, layer scale, identity).  The depthwise conv reads
      fp16(raw32 scale + shift): that operand is restated as float64 -> fp32 -> fp16 (the kernel's fma), and ONE operand per output may
      round the other way (a double rounding on a tie, ~2^-13 of the elements): + 2^-10 max_tap |w tile|.  Attention: softmax
      probabilities carry the relative error of exp at the score's error, HD 2^-24 sum|q k| scale, twice (numerator, denominator), plus
      the 32-term p.v sum: 2^-24 (2 HD max(1, max_k sum_d |q k| scale) + 48) sum_k p |v|.
      The proj_drop expansion outside image rows 0-7 and the attention rows >= 543 are exact.
  MFMA convs on fp16 operands (3x3, 1x1)      4e-3 max(1, |ref|max) per sample (test_conv_forward_and_gn_partials)
  MFMA convs on e4m3 operands (P3)            relative L2 <= 6e-2 per sample (tests/test_fp8_gpu.py)
  (mean, rstd), (scale, shift), running stats  1e-4: |dmean| <= 1e-4 max(1, std), |drstd| <= 1e-4 rstd, |dscale| <= 1e-4 |scale|,
      |dshift| <= 1e-4 |scale| (max(1, std) + |mean|) (shift = beta - mean scale), running_mean as the mean, |d running_var| <= 1e-4 max(1, var)
  pools                                       1e-5 of the mean absolute value of the pooled (sample, channel) column
  heads                                       2e-5 max(1, |ref|max)
  folded attention (o_projc, P0-P3)           4 x the largest difference between the float64 reference without intermediate rounding and
      the one rounded where the plain form rounds (bnA, qkv, attc), + one fp16 ulp at |ref|max: computed from the reference alone

Measured on the MI355X, worst over every layer, block and sample (K1 / K2 / K3 / K4, then P0 / P1 / P2 / P3 where they apply); no
starting bound was exceeded, none was widened, none re-derived:
  round-once kernels        0.4995 / 0.4995 / 0.4995 / 0.4993 of the bound everywhere it is reached: half an fp16 ulp, the rounding itself
                            (block tails and bnA; the first conv 0.498, o_wfus_fold 0.499)
  MFMA convs, fp16          4.5e-4 / 4.3e-4 / 4.0e-4 / 1.2e-4 of max(1, |ref|max) (pointwise edge_branch; K3: conv1 128 -> 256 of block (2,0));
                            P0 / P1 / P2: 3.9e-4 / 3.9e-4 / 2.9e-4 (o_rawA)
  MFMA convs, e4m3 (P3)     relative L2 3.83e-2 (o_rawA, sample 1)
  (mean, rstd)              mean 3e-8 of max(1, std); rstd 6.1e-6 (K1, block (1,2) conv2.2: conv2's output is close to a constant field, its
                            variance is what E[x^2] - mean^2 leaves of fp32 partial sums), 1.9e-7 / 3.5e-7 / 9e-8 in K2 / K3 / K4
  (scale, shift)            1.3e-7 / 1.1e-7 / 1.3e-7 / 1.0e-7 relative; the hand-shake tables o_ss / o_ssb of P0-P3: 2.1e-7 / 2.1e-7 / 2.5e-7 / 2.4e-7
  running statistics        mean 1e-8 of max(1, std), variance 1.4e-7 of max(1, var) (K1-K3 and P0-P3 alike); in the n / (n - 1) form: 0
  pools                     4.0e-7 / 4.0e-7 / 3.7e-7 / 3.8e-7 of the column's mean absolute value; P0-P3: 4.3e-7 / 4.3e-7 / 4.7e-7 / 4.0e-7
  heads                     3.4e-7 / 4.2e-7 / 8.1e-7 / 2.7e-7 of max(1, |ref|max) (an embedding each time; the scores and weights 5e-8)
  folded attention          1.32e-3 / 1.32e-3 / 1.23e-3 / 1.05e-3 against bounds of 6.1e-3 / 6.1e-3 / 5.7e-3 / 6.0e-3 (the plain form's rounding
                            sites move the float64 reference by 1.05e-3 / 1.05e-3 / 9.5e-4 / 1.03e-3: the folded form is as far from the
                            unrounded reference as the plain form is, 0.22 of the yardstick)
  folded fusion operands    o_bfus_fold 6.3e-8 absolute (0.0015 of its bound: 200 fp32 roundings on sum|terms|, 192 products + the tree)
P1 reproduces P0 to the last printed digit: LO_HALO does not reach t_conv3_full (see above).
The tests bite: with one arithmetic-only change at a time on a scratch copy (wrong values, every access in range), failing by assertion --
depthwise halo staged without its leftmost column: test_feature_extractor[K1-K4] (dw[0], 1600 x the bound at column 64 of a tile);
dst_off of the pointwise convs dropped: test_feature_extractor, test_running_statistics, test_folded_fusion_operands; nrow of BatchNorm2's
finalize halved: all 36 test_expert_block[K1-K3] (mrB mean 300-430 x) and test_running_statistics; the tail without id_ss:
test_expert_block[K3-e*l0] (xs); the query token of written position p >= 512 taken one row early (p - 512 for p - 511):
test_expert_block[K1-K3] (attc rows 512-542); inv_keep left off the Dropout2d table: test_expert_block[K2, K3] (bnA) and
test_production_block[P0-P3] (o_ssb, 1000 x); running variance without n / (n - 1): test_running_statistics[K1-K3] (8.8e-6 / 1.7e-5 / 4.4e-5
against 9.5e-7); t_conv3_full reporting lo_igemm_nt's row count on the fused-tap route: test_production_block[P0-P3] (o_ss scale 2.2 for 144).
`pix < 896` for `pix < 1024` in proj_drop changes no value (the compact rows 543 .. 1023 hold fp16(proj.bias), which is what the other
branch writes): an equivalent change, not a gap; `pix < 512` fails all of test_expert_block (a2 rows 0-7) and test_production_block
(o_proj).
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from oracle import dropout_ref as D
from oracle import teacher_ref as T
from oracle import vae_ref as R
from tests.test_teacher_fullgrad_gpu import DROP_P, DROP_SEED

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
E = 4
BANDS = ((0, 8), (60, 68), (120, 128))
ROWS = [r for a, b in BANDS for r in range(a, b)]
U16, S16, E32 = 2.0 ** -10, 2.0 ** -24, 2.0 ** -24          # fp16 ulp (relative), fp16 subnormal spacing, fp32 rounding (relative)
KEPT = {"K1": dict(F=128, B=3, train=True, p=0.0), "K2": dict(F=128, B=2, train=True, p=DROP_P),
        "K3": dict(F=256, B=1, train=True, p=DROP_P), "K4": dict(F=128, B=2, train=False, p=0.0)}
PROD = {"P0": dict(B=2, precision="fp16", halo=None), "P1": dict(B=2, precision="fp16", halo="3"),
        "P2": dict(B=16, precision="fp16", halo=None), "P3": dict(B=2, precision="fp8", halo=None)}
BOUNDS = {"mfma": 4e-3, "mfma_f8": 6e-2, "stat": 1e-4, "pool": 1e-5, "heads": 2e-5}
# space-1 / space-0 kinds of lo_teacher_debug_tensor (include/lunaris_hip.h)
K1_ = dict(raw32=0, dw=1, cat=2, catd=3, rawF=4, feat=5, xs=6, rawA=7, bnA=8, qkv=9, attc=10, projc=11, a2=12, rawB=13, scraw=14, mrA=15,
           mrB=16, mrS=17, ssS=18, mr=19, ssx3=20)
K0_ = dict(raw32=0, cat=1, feat=2, x0=3, x1=4, rawA=5, projc=6, proj=7, rawB=8, ss=9, ssb=10, ss_cat=11, wfus_fold=12, bfus_fold=13)
# running_var once more, in the form of _check_running's last check: the batch variance is E[x^2] - mean^2 in double from fp32 partial
# rows, each the sum of at most 256 squares of fp16 numbers (8 levels of a pairwise sum, 2^-24 each, and as much again for the sum of
# the rows' own roundings): 16 * 2^-24 of E[x^2]; the update's own fp32 roundings (0.9f, 0.1f, one fma, one store) are taken off as
# 2 ulp of the stored value.  Measured: 0 in every layer of K1-K3 (everything lies inside the 2 ulp); the factor n / (n - 1) alone is
# worth 1.9e-5 (batch 3) to 6.1e-5 (batch 1) in the same form
RUN_VAR_N_BOUND = 16 * 2.0 ** -24
WORST = {}          # (configuration, kind) -> (worst error as a fraction of its bound, where)


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def _x(B):
    return R.normalise_sprites(R.closed_form_sprites(B))


@functools.lru_cache(maxsize=None)
def _state(F):
    """the closed-form state (shared: nobody writes into it)"""
    return T.closed_form_teacher_state(**({} if F == 128 else {"feature_dim": F, "embedding_dim": 64}))


def _teacher(F, p, precision="fp16"):
    from lunaris_orion_amd.teacher import LunarMoETeacher
    m = LunarMoETeacher(num_experts=E, feature_dim=F, embedding_dim=64, dropout_rate=p, mfma_precision=precision)
    m.load_state_dict(_state(F))
    return m.to("cuda")


def _view(eng, space, which, e=0, l=0):
    from lunaris_orion_amd import _lib
    off, dims, eb = C.c_size_t(), (C.c_int * 4)(), C.c_int()
    _lib.check(_lib.lib.lo_teacher_debug_tensor(eng.handle, space, which, e, l, C.byref(off), dims, C.byref(eb)), "lo_teacher_debug_tensor")
    shape = tuple(dims)
    n = shape[0] * shape[1] * shape[2] * shape[3] * eb.value
    buf = eng.bws if space else eng.ws
    return buf[off.value:off.value + n].view({2: torch.float16, 4: torch.float32}[eb.value]).view(shape)


def _inv_keep(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def _keep(seed, site, shape, p):
    """keep / (1 - p) of a dropout site in the library's element order (float64, on the device); all ones without dropout"""
    n = int(np.prod(shape))
    if p <= 0:
        return torch.ones(shape, dtype=F64, device="cuda")
    return torch.from_numpy(D.keep_flat(seed, site, n, p)).cuda().to(F64).view(shape) * _inv_keep(p)


def _lrelu(v):
    return torch.where(v > 0, v, 0.2 * v)


def _where(idx, shape):
    return tuple(int(i) for i in np.unravel_index(int(idx), shape))


def _check(cfg, kind, what, got, ref, tol):
    """|got - ref| <= tol elementwise (tol broadcastable); records and prints the worst fraction of the bound; the message names the element"""
    ref = ref.to(F64)
    got = got.to(ref.device, F64)
    err = (got - ref).abs()
    frac = torch.nan_to_num(err / torch.as_tensor(tol, dtype=F64, device=err.device).expand_as(err), nan=0.0)      # 0 / 0: exact where exactness is asked
    bad = ~torch.isfinite(got)
    frac = torch.where(bad, torch.full_like(frac, float("inf")), frac)
    i = int(torch.argmax(frac))
    w = _where(i, tuple(frac.shape))
    f = float(frac.flatten()[i])
    print(f"{cfg} {kind:10s} {what:34s} worst {float(err.flatten()[i]):.3e} = {f:.3f} of its bound at {w}")
    if f > WORST.get((cfg, kind), (-1.0, ""))[0]:
        WORST[(cfg, kind)] = (f, f"{what} {w}")
    assert f <= 1.0, (f"{cfg} {what}: element {w} (sample first) is {float(got.flatten()[i])!r}, reference {float(ref.flatten()[i])!r}: "
                      f"error {float(err.flatten()[i]):.4e} is {f:.3f} of the bound ({kind})")


def _mfma_tol(ref):
    """4e-3 max(1, |ref|max) per sample"""
    m = ref.abs().flatten(1).max(dim=1).values.clamp_min(1.0)
    return (BOUNDS["mfma"] * m).view(-1, *([1] * (ref.dim() - 1)))


def _round_tol(ref, terms, n):
    return U16 * ref.abs() + S16 + n * E32 * terms


def _bands(x):
    return x[:, ROWS]


def _conv_bands(x, w, bias, absolute=False):
    """conv2d (stride 1, zero padding K // 2) of NHWC x with w [Co, Ci, K, K] in float64 on the rows of BANDS: [B, 24, 128, Co]"""
    K, Bn = w.shape[-1], x.shape[0]
    pad = K // 2
    w = w.to(F64)
    outs = []
    for r0, r1 in BANDS:
        lo, hi = r0 - pad, r1 + pad
        xs = x[:, max(lo, 0):min(hi, 128)].to(F64)
        xs = F_.pad(xs, (0, 0, pad, pad, max(0, -lo), max(0, hi - 128)))
        acc = bias.to(F64).view(1, 1, 1, -1).expand(Bn, r1 - r0, 128, w.shape[0]).clone()
        for dy in range(K):
            for dx in range(K):
                acc += xs[:, dy:dy + r1 - r0, dx:dx + 128, :] @ w[:, :, dy, dx].t()
        outs.append(acc)
    return torch.cat(outs, 1)


def _dw_bands(tile, w, bias):
    """depthwise conv of the NHWC tile with w [C, 1, K, K]: (value, sum |terms|, largest |term|) on the rows of BANDS"""
    K, Bn, Cn = w.shape[-1], tile.shape[0], tile.shape[-1]
    pad = K // 2
    w = w.to(F64)
    res = [[], [], []]
    for r0, r1 in BANDS:
        lo, hi = r0 - pad, r1 + pad
        xs = F_.pad(tile[:, max(lo, 0):min(hi, 128)].to(F64), (0, 0, pad, pad, max(0, -lo), max(0, hi - 128)))
        acc = bias.to(F64).view(1, 1, 1, -1).expand(Bn, r1 - r0, 128, Cn).clone()
        tot, big = acc.abs(), torch.zeros_like(acc)
        for dy in range(K):
            for dx in range(K):
                t = xs[:, dy:dy + r1 - r0, dx:dx + 128, :] * w[:, 0, dy, dx]
                acc, tot, big = acc + t, tot + t.abs(), torch.maximum(big, t.abs())
        for k, v in enumerate((acc, tot, big)):
            res[k].append(v)
    return tuple(torch.cat(r, 1) for r in res)


def _stats(raw):
    """float64 (mean, biased variance) per channel of an [..., C] tensor"""
    v = raw.reshape(-1, raw.shape[-1]).to(F64)
    m = v.mean(0)
    return m, ((v * v).mean(0) - m * m).clamp_min(0.0)


def _check_mr(cfg, what, mr, mean, var):
    mr = mr.view(-1, 2).to(F64)
    std, rstd = var.sqrt(), 1.0 / torch.sqrt(var + T.BN_EPS)
    _check(cfg, "mean", what + " mean", mr[:, 0], mean, BOUNDS["stat"] * std.clamp_min(1.0))
    _check(cfg, "rstd", what + " rstd", mr[:, 1], rstd, BOUNDS["stat"] * rstd)


def _check_ss(cfg, what, ss, mean, var, gamma, beta, factor=None):
    """(scale, shift) [C][2] (or, with factor [B, C], the per-sample Dropout2d table [B][C][2]) against gamma rstd and beta - mean scale"""
    std = var.sqrt()
    sc = gamma.to(F64) / torch.sqrt(var + T.BN_EPS)
    sh = beta.to(F64) - mean * sc
    tsc, tsh = BOUNDS["stat"] * sc.abs(), BOUNDS["stat"] * sc.abs() * (std.clamp_min(1.0) + mean.abs()) + 1e-9
    ss = ss.to(F64)
    if factor is not None:
        ss = ss.view(factor.shape[0], -1, 2)
        sc, sh, tsc, tsh = sc * factor, sh * factor, tsc * factor.abs() + 1e-12, tsh * factor.abs() + 1e-12
    else:
        ss = ss.view(-1, 2)
    _check(cfg, "scale", what + " scale", ss[..., 0], sc, tsc)
    _check(cfg, "shift", what + " shift", ss[..., 1], sh, tsh)


def _table(mr, gamma, beta):
    """float64 (scale, shift, sum-of-|terms| helper) from a stored (mean, rstd) table, as lo_bn_finalize_kernel forms them"""
    mr = mr.view(-1, 2).to(F64)
    sc = gamma.to(F64) * mr[:, 1]
    return sc, beta.to(F64) - mr[:, 0] * sc, (mr[:, 0] * sc).abs() + beta.to(F64).abs()


def _check_running(cfg, what, after, name, old, raw, n_old=None):
    """running_mean / running_var after ONE train-mode call = 0.9 old + 0.1 (batch mean, unbiased batch variance) of the stored raw tensor"""
    mean, var = _stats(raw)
    n = raw.numel() // raw.shape[-1]
    rm = 0.9 * old[name + ".running_mean"].cuda().to(F64) + 0.1 * mean
    rv = 0.9 * old[name + ".running_var"].cuda().to(F64) + 0.1 * var * n / (n - 1)
    _check(cfg, "run_mean", what + " running_mean", after[name + ".running_mean"], rm, BOUNDS["stat"] * var.sqrt().clamp_min(1.0))
    _check(cfg, "run_var", what + " running_var", after[name + ".running_var"], rv, BOUNDS["stat"] * var.clamp_min(1.0))
    # the unbiased factor n / (n - 1) is 2e-5 ... 6e-5 of the variance: below the 1e-4 form.  Measured apart, in the form the error of
    # E[x^2] - mean^2 from fp32 partial rows takes: (|d| - 2 fp32 ulp of the stored value) / (0.1 (var + mean^2))
    d = ((after[name + ".running_var"].to(F64) - rv).abs() - 2 * 2.0 ** -23 * rv.abs()).clamp_min(0.0) / (0.1 * (var + mean * mean) + 1e-30)
    effect = (1.0 / (n - 1)) * (var / (var + mean * mean + 1e-30))          # what leaving the factor out would show, same form
    i = int(torch.argmax(d))
    print(f"{cfg} run_var_n  {what:34s} worst {float(d[i]):.3e} of 0.1 E[x^2] at channel {i}; the unbiased factor is worth {float(effect.max()):.3e}")
    if float(d[i]) > WORST.get((cfg, "run_var_n"), (-1.0, ""))[0]:
        WORST[(cfg, "run_var_n")] = (float(d[i]), f"{what} channel {i}")
    if RUN_VAR_N_BOUND is not None:
        assert float(d[i]) <= RUN_VAR_N_BOUND, (cfg, what, i, float(d[i]))


def _attention_ref(qkv, Fd, att_keep):
    """chunk-local attention as executed, from qkv [B, 16384, 3F] (float64): (attc rows 0..542 [B, 543, F], tolerance helper).  Written
    position p < 512 is query token 32 p of chunk p; p >= 512 is token 32 * 511 + (p - 511) of chunk 511.  att_keep: [B, 543, 8, 32]"""
    Bn, HD = qkv.shape[0], Fd // 8
    p = torch.arange(543, device=qkv.device)
    chunk = torch.clamp(p, max=511)
    qtok = torch.where(p < 512, 32 * p, 32 * 511 + (p - 511))
    q = qkv[:, qtok, :Fd].reshape(Bn, 543, 8, HD)
    ktok = (32 * chunk).view(-1, 1) + torch.arange(32, device=qkv.device).view(1, -1)               # [543, 32]
    k = qkv[:, ktok, Fd:2 * Fd].reshape(Bn, 543, 32, 8, HD)
    v = qkv[:, ktok, 2 * Fd:].reshape(Bn, 543, 32, 8, HD)
    s = torch.einsum("bphd,bpkhd->bphk", q, k) * HD ** -0.5
    sabs = torch.einsum("bphd,bpkhd->bphk", q.abs(), k.abs()) * HD ** -0.5
    a = torch.softmax(s, dim=-1) * att_keep
    out = torch.einsum("bphk,bpkhd->bphd", a, v)
    oabs = torch.einsum("bphk,bpkhd->bphd", a, v.abs())
    tol_terms = oabs * (2 * HD * sabs.max(dim=-1).values.clamp_min(1.0) + 48).unsqueeze(-1)
    return out.reshape(Bn, 543, Fd), tol_terms.reshape(Bn, 543, Fd)


def _heads_ref(S, pool_f, pool_e, seed, p, B):
    """float64 gate and heads (oracle/teacher_ref._head in float64) from the stored pooled features; masks of the head sites"""
    S = {k: v.cuda().to(F64) for k, v in S.items() if v.is_floating_point() and k.split(".")[0] in ("gate", "quality_heads", "semantic_head", "style_net", "prompt_net")}
    mk = lambda site, width: _keep(seed, site, (B, width), p) if p > 0 else None
    g = _lrelu(pool_f @ S["gate.2.weight"].t() + S["gate.2.bias"])
    if p > 0:
        g = g * mk(D.DS_GATE, g.shape[1])
    w = torch.softmax(g @ S["gate.5.weight"].t() + S["gate.5.bias"], dim=1)
    rq = torch.stack([T._head(pool_e[e], S, f"quality_heads.{e}", mask=mk(D.ds_quality(e), 64)) for e in range(E)], dim=1)       # [B, E, 4]
    comb = (pool_e.permute(1, 0, 2) * w.unsqueeze(-1)).sum(1)
    return {"raw_q": rq, "expert_weights": w, "quality_scores": torch.sigmoid((rq * w.unsqueeze(-1)).sum(1)),
            "style_embedding": T._head(comb, S, "style_net", mask=mk(D.DS_STYLE, 128)),
            "prompt_embedding": T._head(comb, S, "prompt_net", mask=mk(D.DS_PROMPT, 128)),
            "semantic_score": T._head(pool_e[0], S, "semantic_head", final="sigmoid", mask=mk(D.DS_SEM, 128))}


def _saved(eng):
    pf, pe, rq = eng.saved_views()
    B = eng.batch
    return pf.view(B, 128).to(F64), pe.view(E, B, -1).to(F64), rq.view(B, E, 4).to(F64)


# ---- the kept forward ---------------------------------------------------------------------------------------------------------
class Kept:
    def __init__(self, cfg):
        c = KEPT[cfg]
        self.cfg, self.F, self.B, self.train, self.p = cfg, c["F"], c["B"], c["train"], c["p"]
        self.seed = DROP_SEED if self.p > 0 else 0
        self.S = _state(self.F)                                           # the state that went in (closed form), CPU fp32
        self.m = _teacher(self.F, self.p)
        self.m.train(self.train)
        self.x = _x(self.B).cuda()
        if self.p > 0:
            self.m.set_dropout_stream(DROP_SEED, exact_next=True)
        self.m._ensure_flat()
        before = self.m._flat.clone()
        with torch.no_grad():
            out, self.eng, p, seed = self.m._native_forward(self.x, mode="keep" if self.train else "keep_eval")
        torch.cuda.synchronize()
        assert (p, seed) == ((self.p, self.seed) if self.train else (0.0, 0))
        self.out = {k: v.clone() for k, v in out.items() if torch.is_tensor(v)}
        self.after = {k: v.detach().clone() for k, v in self.m.state_dict().items() if v.is_floating_point()}
        self.flat_unchanged = bool(torch.equal(before, self.m._flat))
        self.ik = _inv_keep(self.p)

    def t(self, name, e=0, l=0):
        return _view(self.eng, 1, K1_[name], e, l)

    def par(self, k):
        return self.S[k].cuda()

    def w16(self, k):
        """a weight the pack rounds through fp16"""
        return self.S[k].cuda().half().to(F64)

    def bn_stats(self, raw, name):
        """what the layer's tables must hold: batch statistics of the stored raw tensor, or (eval) the running statistics"""
        if self.train:
            return _stats(raw)
        return self.par(name + ".running_mean").to(F64), self.par(name + ".running_var").to(F64)


@functools.lru_cache(maxsize=None)
def _kept(cfg):
    return Kept(cfg)


@pytest.fixture(scope="module", params=list(KEPT))
def kept(request):
    return _kept(request.param)


def test_feature_extractor(kept):
    k, cfg, B = kept, kept.cfg, kept.B
    fe = "feature_extractor"
    raw32 = k.t("raw32")
    # raw32 = lrelu(conv 3 -> 32), fp32 weights
    xn = k.x.permute(0, 2, 3, 1)
    w, b = k.par(fe + ".conv1.0.weight"), k.par(fe + ".conv1.0.bias")
    ref = _lrelu(_conv_bands(xn, w, b))
    terms = _conv_bands(xn.abs(), w.abs(), b.abs())
    _check(cfg, "round1", "raw32 (first conv)", _bands(raw32), ref, _round_tol(ref, terms, 28))
    # its BatchNorm: (mean, rstd) and the (scale, shift) the depthwise convs read
    mean, var = k.bn_stats(raw32, fe + ".conv1.2")
    _check_mr(cfg, "conv1.2", k.t("mr", 0, 3), mean, var)
    ss32 = k.t("ssx3")
    _check_ss(cfg, "conv1.2", ss32, mean, var, k.par(fe + ".conv1.2.weight"), k.par(fe + ".conv1.2.bias"))
    # the depthwise convs read fp16(raw32 scale + shift) with zero padding of the normalised tensor
    ss = ss32.view(32, 2).to(F64)
    tile = (raw32.to(F64) * ss[:, 0] + ss[:, 1]).float().half()
    cat, refs = k.t("cat"), []
    for bi, br in enumerate(("edge_branch", "color_branch", "detail_branch")):
        q = f"{fe}.{br}"
        K = 5 if bi == 1 else 3
        ref, terms, big = _dw_bands(tile, k.par(q + ".0.weight"), k.par(q + ".0.bias"))
        dw = k.t("dw", 0, bi)
        _check(cfg, "round1", f"dw[{bi}] ({K}x{K} depthwise)", _bands(dw), ref, _round_tol(ref, terms, K * K + 1) + U16 * big)
        # pointwise 32 -> 64 + LeakyReLU, in its own 64-channel slice of cat
        ref = _lrelu(dw.to(F64) @ k.w16(q + ".1.weight").view(64, 32).t() + k.par(q + ".1.bias").to(F64))
        refs.append(ref)
        sl = cat[..., 64 * bi:64 * bi + 64]
        _check(cfg, "mfma", f"cat[{64 * bi}:{64 * bi + 64}] (pointwise {br})", sl, ref, _mfma_tol(ref))
        mean, var = k.bn_stats(sl, q + ".3")
        _check_mr(cfg, br + ".3", k.t("mr", 0, 4 + bi), mean, var)
        _check_ss(cfg, br + ".3", _view(k.eng, 0, K0_["ss_cat"]).view(192, 2)[64 * bi:64 * bi + 64], mean, var, k.par(q + ".3.weight"), k.par(q + ".3.bias"))
    # a slice holds nothing of another branch: every slice is far from the other two branches' references (so the check above tells them apart)
    for bi in range(3):
        for bj in range(3):
            if bi != bj:
                d = (cat[..., 64 * bi:64 * bi + 64].to(F64) - refs[bj]).abs().max().item()
                assert d > 25 * BOUNDS["mfma"] * max(1.0, refs[bj].abs().max().item()), (cfg, bi, bj, d)
    # catd = Dropout(BN(cat)) with the mask of site LO_DS_FE (element index pix * 192 + c)
    sc = _view(k.eng, 0, K0_["ss_cat"]).view(192, 2).to(F64)
    keep = _keep(k.seed, D.DS_FE, (B, 128, 128, 192), k.p if k.train else 0.0)
    v = cat.to(F64) * sc[:, 0] + sc[:, 1]
    terms = ((cat.to(F64) * sc[:, 0]).abs() + sc[:, 1].abs()) * keep
    catd = k.t("catd")
    _check(cfg, "round1", "catd = Dropout(BN(cat))", catd, v * keep, _round_tol(v * keep, terms, 8))
    if k.p > 0 and k.train:
        assert bool((catd[keep == 0] == 0).all()) and 0.05 < float((keep == 0).double().mean()) < 0.15
    # fusion conv 192 -> 128 + LeakyReLU, its BatchNorm, feat, the pooled features
    ref = _lrelu(catd.to(F64) @ k.w16(fe + ".fusion.0.weight").view(128, 192).t() + k.par(fe + ".fusion.0.bias").to(F64))
    rawF = k.t("rawF")
    _check(cfg, "mfma", "rawF (fusion conv)", rawF, ref, _mfma_tol(ref))
    mean, var = k.bn_stats(rawF, fe + ".fusion.2")
    mrF = k.t("mr", 0, 7)
    _check_mr(cfg, "fusion.2", mrF, mean, var)
    sc, sh, tb = _table(mrF, k.par(fe + ".fusion.2.weight"), k.par(fe + ".fusion.2.bias"))
    ref = rawF.to(F64) * sc + sh
    feat = k.t("feat")
    _check(cfg, "round1", "feat = BN(rawF)", feat, ref, _round_tol(ref, (rawF.to(F64) * sc).abs() + tb, 8))
    pf = _saved(k.eng)[0]
    fm = feat.to(F64).view(B, T_HW, 128)
    _check(cfg, "pool", "o_pool_f", pf, fm.mean(1), BOUNDS["pool"] * fm.abs().mean(1) + 1e-30)


T_HW = 16384
BLOCKS = [(e, l) for e in range(E) for l in range(3)]


@pytest.mark.parametrize("e,l", BLOCKS, ids=[f"e{e}l{l}" for e, l in BLOCKS])
def test_expert_block(kept, e, l):
    k, cfg, B, Fd = kept, kept.cfg, kept.B, kept.F
    p = k.p if k.train else 0.0
    pre, blk = f"experts.{e}.{l}", f"block ({e},{l}) "
    xin = k.t("feat") if l == 0 else k.t("xs", e, l - 1)
    cin = xin.shape[-1]
    sc_branch = Fd != 128 and l == 0
    ident, ident_terms = xin.to(F64), xin.to(F64).abs()
    if sc_branch:
        # shortcut = BatchNorm(Conv1x1(x)): the raw conv is stored, its (scale, shift) is applied inside the tail
        ref = xin.to(F64) @ k.w16(pre + ".shortcut.0.weight").view(Fd, cin).t() + k.par(pre + ".shortcut.0.bias").to(F64)
        scraw = k.t("scraw", e, l)
        _check(cfg, "mfma", blk + "scraw (shortcut 1x1)", scraw, ref, _mfma_tol(ref))
        mean, var = k.bn_stats(scraw, pre + ".shortcut.1")
        _check_mr(cfg, blk + "shortcut.1 mrS", k.t("mrS", e, l), mean, var)
        ssS = k.t("ssS", e, l)
        _check_ss(cfg, blk + "shortcut.1 ssS", ssS, mean, var, k.par(pre + ".shortcut.1.weight"), k.par(pre + ".shortcut.1.bias"))
        s2 = ssS.view(Fd, 2).to(F64)
        ident, ident_terms = scraw.to(F64) * s2[:, 0] + s2[:, 1], (scraw.to(F64) * s2[:, 0]).abs() + s2[:, 1].abs()
    # conv1 + LeakyReLU, BatchNorm1 (+ Dropout2d on the table)
    ref = _lrelu(_conv_bands(xin, k.w16(pre + ".conv1.0.weight"), k.par(pre + ".conv1.0.bias")))
    rawA = k.t("rawA", e, l)
    _check(cfg, "mfma", blk + "rawA (conv1 3x3)", _bands(rawA), ref, _mfma_tol(ref))
    mean, var = k.bn_stats(rawA, pre + ".conv1.2")
    mrA = k.t("mrA", e, l)
    _check_mr(cfg, blk + "conv1.2 mrA", mrA, mean, var)
    sc, sh, tb = _table(mrA, k.par(pre + ".conv1.2.weight"), k.par(pre + ".conv1.2.bias"))
    f1 = _keep(k.seed, D.ds_block(e, l, 0), (B, 1, 1, Fd), p)
    ref = (rawA.to(F64) * sc + sh) * f1
    bnA = k.t("bnA", e, l)
    _check(cfg, "round1", blk + "bnA = Dropout2d(BN(rawA))", bnA, ref, _round_tol(ref, ((rawA.to(F64) * sc).abs() + tb) * f1, 8))
    # qkv
    ref = bnA.to(F64) @ k.w16(pre + ".attention.qkv.weight").view(3 * Fd, Fd).t() + k.par(pre + ".attention.qkv.bias").to(F64)
    qkv = k.t("qkv", e, l)
    _check(cfg, "mfma", blk + "qkv (1x1)", qkv, ref, _mfma_tol(ref))
    # attention on the compact rows: rows < 543 (512 .. 542: the single-token queries of chunk 511), rows >= 543 exactly zero
    ak = _keep(k.seed, D.ds_block(e, l, 1), (B, 543, 8, 32), p)
    ref, terms = _attention_ref(qkv.to(F64).view(B, T_HW, 3 * Fd), Fd, ak)
    attc = k.t("attc", e, l).view(B, 1024, Fd)
    _check(cfg, "round1", blk + "attc rows < 543", attc[:, :543], ref, U16 * ref.abs() + S16 + E32 * terms)
    assert int(torch.count_nonzero(attc[:, 543:])) == 0, f"{cfg} {blk}attc: rows >= 543 are not exactly zero"
    # proj on the compact rows
    ref = attc.to(F64) @ k.w16(pre + ".attention.proj.weight").view(Fd, Fd).t() + k.par(pre + ".attention.proj.bias").to(F64)
    projc = k.t("projc", e, l).view(B, 1024, Fd)
    _check(cfg, "mfma", blk + "projc (proj 1x1, compact)", projc, ref, _mfma_tol(ref))
    # a2 = proj_drop of the expansion: image rows 0..7 from projc, fp16(proj.bias) elsewhere (exact), element index (b HW + pix) F + c
    pk = _keep(k.seed, D.ds_block(e, l, 2), (B, T_HW, Fd), p)
    a2 = k.t("a2", e, l).view(B, T_HW, Fd)
    ref = projc.to(F64) * pk[:, :1024]
    _check(cfg, "round1", blk + "a2 rows 0-7 (proj_drop)", a2[:, :1024], ref, _round_tol(ref, ref.abs(), 1))
    bias16 = k.par(pre + ".attention.proj.bias").half()
    rest = torch.where(pk[:, 1024:] > 0, (bias16.float() * torch.tensor(k.ik if p > 0 else 1.0, dtype=torch.float32, device="cuda")).half(), torch.zeros_like(bias16))
    neq = a2[:, 1024:] != rest
    assert not bool(neq.any()), (f"{cfg} {blk}a2 outside image rows 0-7: {int(neq.sum())} elements differ from fp16(fp16(proj.bias) / (1 - p)) or 0, "
                                 f"first at {_where(int(torch.nonzero(neq.flatten())[0]), tuple(neq.shape))}")
    # conv2 + LeakyReLU, BatchNorm2, the tail
    ref = _lrelu(_conv_bands(a2.view(B, 128, 128, Fd), k.w16(pre + ".conv2.0.weight"), k.par(pre + ".conv2.0.bias")))
    rawB = k.t("rawB", e, l)
    _check(cfg, "mfma", blk + "rawB (conv2 3x3)", _bands(rawB), ref, _mfma_tol(ref))
    mean, var = k.bn_stats(rawB, pre + ".conv2.2")
    mrB = k.t("mrB", e, l)
    _check_mr(cfg, blk + "conv2.2 mrB", mrB, mean, var)
    sc, sh, tb = _table(mrB, k.par(pre + ".conv2.2.weight"), k.par(pre + ".conv2.2.bias"))
    f2 = _keep(k.seed, D.ds_block(e, l, 3), (B, 1, 1, Fd), p)
    ls = k.par(pre + ".layer_scale").view(Fd).to(F64)
    ref = _lrelu((rawB.to(F64) * sc + sh) * f2 * ls + ident)
    terms = ((rawB.to(F64) * sc).abs() + tb) * f2 * ls.abs() + ident_terms
    xs = k.t("xs", e, l)
    _check(cfg, "round1", blk + "xs (tail)", xs, ref, _round_tol(ref, terms, 8))
    if l == 2:
        pe = _saved(k.eng)[1][e]
        xm = xs.to(F64).view(B, T_HW, Fd)
        _check(cfg, "pool", f"o_pool_e[{e}]", pe, xm.mean(1), BOUNDS["pool"] * xm.abs().mean(1) + 1e-30)


def _bn_layers(k):
    """(state-dict prefix, stored raw tensor) of every BatchNorm layer of the kept forward"""
    fe = "feature_extractor"
    out = [(fe + ".conv1.2", k.t("raw32"))]
    for bi, br in enumerate(("edge_branch", "color_branch", "detail_branch")):
        out.append((f"{fe}.{br}.3", k.t("cat")[..., 64 * bi:64 * bi + 64]))
    out.append((fe + ".fusion.2", k.t("rawF")))
    for e, l in BLOCKS:
        pre = f"experts.{e}.{l}"
        out += [(pre + ".conv1.2", k.t("rawA", e, l)), (pre + ".conv2.2", k.t("rawB", e, l))]
        if k.F != 128 and l == 0:
            out.append((pre + ".shortcut.1", k.t("scraw", e, l)))
    return out


def test_running_statistics(kept):
    k = kept
    if not k.train:
        assert k.flat_unchanged, "K4: lo_teacher_forward_keep_eval changed the flat state"
        for name, v in k.after.items():
            assert torch.equal(v.cpu(), k.S[name]), name
        return
    assert not k.flat_unchanged
    layers = _bn_layers(k)
    assert len(layers) == (29 if k.F == 128 else 29 + E)
    for name, raw in layers:
        _check_running(k.cfg, name, k.after, name, k.S, raw)
    # nothing but running statistics moved
    for name, v in k.after.items():
        if "running_" not in name:
            assert torch.equal(v.cpu(), k.S[name]), name


def test_heads(kept):
    k = kept
    pf, pe, rq = _saved(k.eng)
    ref = _heads_ref(k.S, pf, pe, k.seed, k.p if k.train else 0.0, k.B)
    for name in ("quality_scores", "expert_weights", "style_embedding", "prompt_embedding", "semantic_score"):
        _check(k.cfg, "heads", name, k.out[name], ref[name], BOUNDS["heads"] * max(1.0, ref[name].abs().max().item()))
    _check(k.cfg, "heads", "raw_q", rq, ref["raw_q"], BOUNDS["heads"] * max(1.0, ref["raw_q"].abs().max().item()))


# ---- the production route: lo_teacher_forward, path 2, block (E-1, 2) in its own workspace -------------------------------------------
def _psamples(B):
    if B < 4:
        return list(range(B))
    i = (37 * B) // 64 | 1
    return [0, i, B - 1]


def _prof_names():
    from lunaris_orion_amd import _lib
    names, name = [], C.create_string_buffer(128)
    ms, fl, by = C.c_double(), C.c_double(), C.c_double()
    for i in range(_lib.lib.lo_prof_count()):
        _lib.lib.lo_prof_get(i, name, 128, C.byref(ms), C.byref(fl), C.byref(by))
        names.append(name.value.decode())
    return names


def _capture_prod(B, precision):
    """One train-mode lo_teacher_forward with dropout on a fresh model, and what block (E-1, 2) left in the workspace, on the CPU"""
    from lunaris_orion_amd import _lib
    lib = _lib.lib
    m = _teacher(128, DROP_P, precision)
    m.train()
    m.set_dropout_stream(DROP_SEED, exact_next=True)
    x = _x(B).cuda()
    m._ensure_flat()
    eng = m._engine(B)
    lib.lo_prof_enable(1)
    try:
        with torch.no_grad():
            out, eng2, p, seed = m._native_forward(x)
        torch.cuda.synchronize()
        names = _prof_names()
    finally:
        lib.lo_prof_enable(0)
    assert eng2 is eng and (p, seed) == (DROP_P, DROP_SEED)
    S = _psamples(B)
    v = lambda name: _view(eng, 0, K0_[name])
    pre = f"experts.{E - 1}.2"
    cap = {"B": B, "samples": S, "precision": precision, "path": int(lib.lo_teacher_last_path(eng.handle)), "names": names,
           "out": {k: t.cpu() for k, t in out.items() if torch.is_tensor(t)},
           "after": {k: t.detach().cpu().clone() for k, t in m.state_dict().items() if "running_" in k and k.startswith(pre)},
           "ss": v("ss").cpu().clone(), "ssb": v("ssb").cpu().clone(), "pool_e": eng.saved_views()[1].view(E, B, 128)[E - 1].cpu().clone()}
    for name in ("x1", "rawA", "proj", "rawB"):
        cap[name] = v(name)[S].cpu().clone()
    cap["projc"] = v("projc")[S].cpu().clone()
    # whole-batch facts the per-sample tensors cannot give: float64 statistics of the stored raw tensors, on the device
    for name in ("rawA", "rawB"):
        cap[name + "_stats"] = tuple(t.cpu() for t in _stats(v(name)))
    # the tail's pooled sum needs every sample's rawB and x1: the float64 column mean of the restated tail, on the device
    ssb = v("ssb").view(B, 1, 128, 2).to(F64)
    ls = _state(128)[pre + ".layer_scale"].cuda().view(128).to(F64)
    tail = _lrelu((v("rawB").view(B, T_HW, 128).to(F64) * ssb[..., 0] + ssb[..., 1]) * ls + v("x1").view(B, T_HW, 128).to(F64)).half().to(F64)
    cap["tail_mean"], cap["tail_absmean"] = tail.mean(1).cpu(), tail.abs().mean(1).cpu()
    # which kernel: the op-level entry of the fused-tap kernel on the stored input must give the stored o_rawA bit for bit
    if precision == "fp16":
        w = _state(128)[pre + ".conv1.0.weight"].cuda().contiguous()
        n = lib.lo_packed_weight_elems_for(0, B, 128, 128, 128, 128)
        wp = torch.empty(n, dtype=torch.float16, device="cuda")
        _lib.check(lib.lo_pack_weight_for(0, B, 128, 128, 128, 128, w.data_ptr(), wp.data_ptr(), _lib.stream_ptr()), "lo_pack_weight_for")
        bias = _state(128)[pre + ".conv1.0.bias"].cuda().contiguous()
        again = torch.full((B, 128, 128, 128), float("nan"), dtype=torch.float16, device="cuda")
        part = torch.zeros(B * 64 * 128 * 2, dtype=torch.float32, device="cuda")
        _lib.check(lib.lo_conv3x3_fused_tap_forward(B, 128, 128, 128, 128, 0, v("x1").data_ptr(), wp.data_ptr(), None, bias.data_ptr(), 1,
                                                    again.data_ptr(), part.data_ptr(), _lib.stream_ptr()), "lo_conv3x3_fused_tap_forward")
        torch.cuda.synchronize()
        cap["fused_tap_bitwise"] = bool(torch.equal(again, v("rawA")))
    del eng, eng2, m
    torch.cuda.empty_cache()
    return cap


_CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
from tests.test_teacher_insitu_gpu import _capture_prod
torch.save(_capture_prod({B}, {precision!r}), sys.argv[1])
print("TEACHER_INSITU_CAPTURED")
"""


@functools.lru_cache(maxsize=None)
def _prod_run(cfg, tmpdir):
    c = PROD[cfg]
    if c["halo"] is None:
        return _capture_prod(c["B"], c["precision"])
    f = os.path.join(tmpdir, f"teacher_insitu_{cfg}.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, B=c["B"], precision=c["precision"]), f],
                       env=dict(os.environ, LO_HALO=c["halo"]), capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "TEACHER_INSITU_CAPTURED" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    return torch.load(f)


def _to_cuda(o):
    if torch.is_tensor(o):
        return o.cuda()
    if isinstance(o, dict):
        return {k: _to_cuda(v) for k, v in o.items()}
    if isinstance(o, tuple):
        return tuple(_to_cuda(v) for v in o)
    return o


@pytest.fixture(scope="module", params=list(PROD))
def prod(request, tmp_path_factory):
    cap = _prod_run(request.param, str(tmp_path_factory.getbasetemp()))
    return request.param, _to_cuda(cap)


def test_production_route_takes_the_kernel_it_is_said_to(prod):
    cfg, c = prod
    f8 = c["precision"] == "fp8"
    assert c["path"] == 2
    tag = " (dense, dropout path, e4m3)" if f8 else " (dense, dropout path)"
    assert c["names"].count("t_conv1" + tag) == 12 and c["names"].count("t_conv2" + tag) == 12, sorted(set(c["names"]))
    other = " (dense, dropout path)" if f8 else " (dense, dropout path, e4m3)"
    assert not any(n.endswith(other) for n in c["names"])
    assert "lo_t_attn_folded" in c["names"] and "lo_t_projdrop" in c["names"] and not any("attn (generic)" in n for n in c["names"])
    if not f8:
        assert c["fused_tap_bitwise"], f"{cfg}: o_rawA is not what lo_conv3x3_fused_tap_forward gives on the stored o_x1"


def _rel_l2(got, ref):
    d = (got.to(F64) - ref).flatten(1)
    return d.norm(dim=1) / ref.flatten(1).norm(dim=1).clamp_min(1e-30)


def _check_conv_prod(cfg, c, what, got, ref):
    if c["precision"] == "fp8":
        r = _rel_l2(got, ref)
        _check(cfg, "mfma_f8", what + " relative L2", r, torch.zeros_like(r), BOUNDS["mfma_f8"])
    else:
        _check(cfg, "mfma", what, got, ref, _mfma_tol(ref))


def _expand(projc, bias, pk, ik):
    """the proj_drop expansion as the kernel forms it, exactly: fp16(fp32(v) * fp32(1 / (1 - p))) or 0"""
    n = projc.shape[0]
    full = bias.half().view(1, 1, -1).expand(n, T_HW, -1).clone()
    full[:, :1024] = projc.view(n, 1024, -1)
    v = (full.float() * torch.tensor(ik, dtype=torch.float32, device=full.device)).half()
    return torch.where(pk > 0, v, torch.zeros_like(v))


def test_production_block(prod):
    cfg, c = prod
    B, smp, f8 = c["B"], c["samples"], c["precision"] == "fp8"
    S = _state(128)
    e, l = E - 1, 2
    pre = f"experts.{e}.{l}"
    par = lambda k_: S[pre + k_].cuda()
    w16 = lambda k_: S[pre + k_].cuda().half().to(F64)
    ik, ns = _inv_keep(DROP_P), len(smp)
    # conv1 of the stored x2
    ref = _lrelu(_conv_bands(c["x1"], w16(".conv1.0.weight"), par(".conv1.0.bias")))
    _check_conv_prod(cfg, c, "o_rawA (conv1 of o_x1)", _bands(c["rawA"]), ref)
    # proj_drop expansion of the stored o_projc (in fp8 mode the kernel writes the e4m3 copy only: o_proj is not written, the
    # restated expansion stands in for it as conv2's unquantised input)
    pk_all = _keep(DROP_SEED, D.ds_block(e, l, 2), (B, T_HW, 128), DROP_P)
    exp = _expand(c["projc"], par(".attention.proj.bias"), pk_all[smp], ik)
    if not f8:
        neq = c["proj"].view(ns, T_HW, 128) != exp
        assert not bool(neq.any()), f"{cfg} o_proj: {int(neq.sum())} elements differ from the proj_drop expansion of the stored o_projc"
    a2 = exp if f8 else c["proj"].view(ns, T_HW, 128)
    ref = _lrelu(_conv_bands(a2.view(ns, 128, 128, 128), w16(".conv2.0.weight"), par(".conv2.0.bias")))
    _check_conv_prod(cfg, c, "o_rawB (conv2 of o_proj)", _bands(c["rawB"]), ref)
    # THE hand-shake: the (scale, shift) left in o_ss for BatchNorm2 -- built from the partial rows the conv epilogue wrote and the row
    # count t_conv3_full reported -- against the float64 statistics of the stored o_rawB over the whole batch
    mean, var = c["rawB_stats"]
    _check_ss(cfg, "o_ss (BatchNorm2 of the last block)", c["ss"], mean, var, par(".conv2.2.weight"), par(".conv2.2.bias"))
    f2 = _keep(DROP_SEED, D.ds_block(e, l, 3), (B, 128), DROP_P)
    _check_ss(cfg, "o_ssb (its Dropout2d table)", c["ssb"], mean, var, par(".conv2.2.weight"), par(".conv2.2.bias"), factor=f2)
    # running statistics of both BatchNorms
    for bn, raw in ((".conv1.2", "rawA"), (".conv2.2", "rawB")):
        mean_, var_ = c[raw + "_stats"]
        n = B * T_HW
        rm = 0.9 * par(bn + ".running_mean").to(F64) + 0.1 * mean_
        rv = 0.9 * par(bn + ".running_var").to(F64) + 0.1 * var_ * n / (n - 1)
        _check(cfg, "run_mean", pre + bn + " running_mean", c["after"][pre + bn + ".running_mean"], rm, BOUNDS["stat"] * var_.sqrt().clamp_min(1.0))
        _check(cfg, "run_var", pre + bn + " running_var", c["after"][pre + bn + ".running_var"], rv, BOUNDS["stat"] * var_.clamp_min(1.0))
    # pooled tail: every element rounded to fp16 before it is summed
    _check(cfg, "pool", f"o_pool_e[{e}]", c["pool_e"], c["tail_mean"], BOUNDS["pool"] * c["tail_absmean"] + 1e-30)
    # folded attention: o_projc against float64 proj(attention(qkv(Dropout2d(BN(rawA))))) of the stored o_rawA
    mean, var = c["rawA_stats"]
    sc = par(".conv1.2.weight").to(F64) / torch.sqrt(var + T.BN_EPS)
    sh = par(".conv1.2.bias").to(F64) - mean * sc
    f1 = _keep(DROP_SEED, D.ds_block(e, l, 0), (B, 1, 1, 128), DROP_P)[smp]
    ak = _keep(DROP_SEED, D.ds_block(e, l, 1), (B, 543, 8, 32), DROP_P)[smp]
    wq, bq = w16(".attention.qkv.weight").view(384, 128), par(".attention.qkv.bias").to(F64)
    wp, bp = w16(".attention.proj.weight").view(128, 128), par(".attention.proj.bias").to(F64)

    def chain(rnd):
        r = (lambda t: t.half().to(F64)) if rnd else (lambda t: t)
        bnA = r((c["rawA"].to(F64) * sc + sh) * f1)
        qkv = r(bnA.view(ns, T_HW, 128) @ wq.t() + bq)
        att = torch.zeros(ns, 1024, 128, dtype=F64, device="cuda")
        att[:, :543] = r(_attention_ref(qkv, 128, ak)[0])
        return att @ wp.t() + bp

    exact, rounded = chain(False), chain(True)
    spread = (exact - rounded).abs().max().item()
    tol = 4 * spread + U16 * exact.abs().max().item()
    print(f"{cfg} folded attention yardstick: plain-form rounding moves the reference by {spread:.3e}; bound {tol:.3e}")
    _check(cfg, "folded", "o_projc (folded attention)", c["projc"].view(ns, 1024, 128), exact, tol)


def test_folded_fusion_operands():
    """A dropout-free train call at batch 2 (path 0): o_wfus_fold = fp16(W scale), o_bfus_fold = b + W shift, from the stored o_ss_cat"""
    from lunaris_orion_amd import _lib
    m = _teacher(128, 0.0)
    m.train()
    with torch.no_grad():
        _, eng, _, _ = m._native_forward(_x(2).cuda())
    torch.cuda.synchronize()
    assert int(_lib.lib.lo_teacher_last_path(eng.handle)) in (0, 1)
    S = _state(128)
    W = S["feature_extractor.fusion.0.weight"].cuda().view(128, 192).to(F64)
    b = S["feature_extractor.fusion.0.bias"].cuda().to(F64)
    ss = _view(eng, 0, K0_["ss_cat"]).view(192, 2).to(F64)
    ref = W * ss[:, 0]
    _check("fold", "round1", "o_wfus_fold = fp16(W scale)", _view(eng, 0, K0_["wfus_fold"]).view(128, 192), ref, _round_tol(ref, ref.abs(), 1))
    ref = b + W @ ss[:, 1]
    terms = b.abs() + W.abs() @ ss[:, 1].abs()
    _check("fold", "fold_bias", "o_bfus_fold = b + W shift", _view(eng, 0, K0_["bfus_fold"]).view(128), ref, 200 * E32 * terms)
    # and the table itself against the float64 statistics of the raw concatenation the same call left in o_cat
    cat = _view(eng, 0, K0_["cat"])
    mean, var = _stats(cat)
    g = torch.cat([S[f"feature_extractor.{br}.3.weight"] for br in ("edge_branch", "color_branch", "detail_branch")]).cuda()
    be = torch.cat([S[f"feature_extractor.{br}.3.bias"] for br in ("edge_branch", "color_branch", "detail_branch")]).cuda()
    _check_ss("fold", "o_ss_cat", _view(eng, 0, K0_["ss_cat"]), mean, var, g, be)


def test_zz_report():
    """Prints the worst figure per configuration and kind (a fraction of its bound) that the tests above measured in this session."""
    for (cfg, kind), (f, where) in sorted(WORST.items()):
        print(f"WORST {cfg:5s} {kind:10s} {f:.4f} of its bound at {where}")
