"""In-situ layer parity of the VAE step: every conv + GroupNorm layer against a plain reference of ITS OWN stored operands.

The conv, GroupNorm and weight-gradient kernels are chosen per geometry and batch; the op-level tests (tests/test_ops_gpu.py,
tests/test_fp8_gpu.py) run at batch 1-8, where the choosers pick the 64 x 64 lo_igemm_nt tile and the small weight-gradient plans.
The benchmarked step runs at batch 64 on other code: 128 x 128 / 128 x 64 tiles, lo_conv3x3_pp with the fused GroupNorm-backward
epilogue (with and without the apply form), the patch-resident transposed conv, the split-K 8 x 8 stage with its fused slab pass,
other weight-gradient split plans -- with epilogues and fusions the op entry points cannot request.  Here one step runs, every
layer's tensors are read out of the workspace (lo_vae_debug_tensor_ex) and each layer is checked on its own: conv, GroupNorm and
their data gradients are per sample, so three samples of a batch-64 layer cost the CPU what a batch-3 op test costs, and the kernel,
tile, epilogue and fusion under test are the ones the step selected.

Configurations: (A) batch 64, fp16; (B) batch 64, mfma_precision="fp8"; (C) batch 2, fp16, LO_HALO=3; (D) batch 2, fp8, LO_HALO=3
(the smallest shape with the fused-tap kernel -- and where, before the plan took the partial-sum row count from the launch the layer
really has, the e4m3 launch wrote 16 / 4 rows per sample where lo_gn_fwd read 8 / 2).  LO_HALO is read once per process: (C) and (D)
run in a fresh child process that saves what it read.  Latent 64: the convs do not depend on it and the Linear layers stay small.
Samples 0, 37, 63 at batch 64 (first, interior odd, last), both at batch 2.

The plan is a function of the batch size, and (A), (B) see one value of it.  The further configurations "fp16-<batch>" / "fp8-<batch>"
(default knobs, in-process, one after the other: each frees its model and workspace, 4 GB at batch 128) run at the batch sizes of
tests/test_vae_plan_cover.py's INSITU_BATCHES, which that module proves on the CPU to launch every layer in every way batch 1..128
does (lo_vae_layer_plan_ex; what it reports is printed beside every figure here).  What each adds, fp16:
    1   the 8 x 8 stage on one 64 x 64-tile launch with the fused GroupNorm-backward apply, one-split weight gradients of 2 K units
    2   the same stage split-K x4 / x9 (128 rows: one M tile), one-split weight gradients (default knobs: (C) forces the fused-tap kernel)
    5   64 x 64 layers: the fused apply off (320 tiles > 256 CUs), weight gradient with all 160 slabs launched
    7   32 x 32 layers: 64 x 64 tiles with the fused apply beside a weight gradient that launches 39 of 42 slabs
    9   32 x 32 layers: the apply off; 16 x 16 ResBlock weight gradient with 9 of 10 slabs and even splits
   10   64 x 64 / 32 x 32 ResBlock weight gradients with dropped splits AND even splits (160 / 170 x 8, 40 / 42 x 8)
   16   lo_conv3x3_pp 16 x 16 x 64 by default, with the fused apply (256 tiles = 256 CUs), first conv applied in conv1's epilogue;
        enc1.0's data gradient on 128 x 64; dec2's on 64 x 64 beside 32 P1 rows
   32   BASELINE config 2: lo_conv3x3_pp 8 x 16 x 128 with the apply (256 tiles), enc1.0's dv written by conv1's epilogue; the
        patch-resident stride-2 data gradient at its threshold; 128 x 64 forward tiles; the 8 x 8 stage split-K x8
   40   split-K x7 on the 8 x 8 stage: 72 K steps, a last split of 6
   45   odd batch above the thresholds: the 8 x 8 stage off split-K (M % 128 != 0) with the apply-only GroupNorm backward
   46   lo_conv3x3_pp 8 x 16 x 128 without the apply beside a weight gradient with 41 of 42 slabs; split-K x6 (and x3 on enc2 / dec1)
   56   split-K x5
   65   odd batch above 64: enc3.0's data gradient on 64 x 128 beside the one-launch forward
   96   split-K x3 on the 8 x 8 stage
  128   128 x 128 forward / data-gradient tiles, 64 x 128 on the 8 x 8 stage, lo_conv3x3_pp 16 x 16 x 128 with ONE tile per sample
fp8 (forward): 2 the 64 x 64 e4m3 tiles; 32 128 x 64 with 8 rows per sample; 128 128 x 128 and 64 x 128.
Samples: first, one odd interior, last ((37 B // 64) | 1: 37 at batch 64), every sample below batch 4.

Forward (A-D), the 12 encoder layers behind the first conv and the 4 transposed convs (the first conv's statistics and output are
checked too; its conv and the final conv have op tests at their only shape):
  statistics  o_stats[n] against the fp64 mean and 1 / sqrt(var + 1e-5) of the stored fp16 v[n]: |dmean| <= 1e-4 max(1, std),
              |drstd| <= 1e-4 rstd (the project's rtol for the partial sums).  Independent of the operand mode; pins the conv
              epilogue -> GroupNorm row hand-shake;
  output      a / stage output / skip form against the same expression in fp64 from the stored v and the stored other operand:
              3e-3 max(1, |y|max) (test_gn_mish_forward_backward);
  conv        v[n] against conv2d / conv_transpose2d (+ bias) in fp64 of the stored input [n], weights rounded through fp16 as the
              pack does: 4e-3 max(1, |ref|max) (test_conv_forward_and_gn_partials); layers on e4m3 operands: relative L2 <= 6e-2
              per sample against the same fp64 conv of the unquantised input (tests/test_fp8_gpu.py).
Backward (A, C); dv carries the step's loss scale (taken from the stepper), parameter gradients come out unscaled:
  weight / bias gradients, whole batch   8 x 8 (cout, cin) pairs (fixed seed) x all taps against the fp64 weight gradient of the
              stored layer input and the stored dv; the conv bias gradient against the fp64 sum of dv: relative L2 <= 2e-4
              (test_conv_wgrad).  All 16 layers, the first conv included (21 x 3 pairs);
  encoder chain   enc[s][1].dv[n] against the fp64 autograd of mish(GN(v1)) seeded with conv2d_input(enc[s][2].dv[n], W): the
              stride-1 data gradient with the fused reduce, with the fused apply, without it on the two-round grid, split-K + slab;
  decoder chain   skipg[3-s][n] against the transposed conv's input gradient of dec[s].dv[n], and dec[s-1].dv[n] against the
              GroupNorm + Mish backward seeded with it: relative L2 <= 3e-3 per tensor and sample (the op test's bound for dv).
The two Linear weight gradients are not read here: xflat / dml / z / Gfc are not among the tensors the debug query names, and the
stepper keeps those gradients factored (tests/test_lowrank_gpu.py checks them).

No bound is derived from an fp8 configuration.  Measured on MI355X, worst layer and sample over all 22 configurations: statistics
1.8e-8 (mean; (B) enc2.0) / 1.2e-7 (rstd; fp16-128 enc3.0); output 4.8e-4 (fp16-32 dec2); conv 4.7e-4 on fp16 operands (fp16-40
enc3.2, split-K x7), relative L2 3.8e-2 on e4m3 operands (fp8-2 dec1); weight / bias gradient 2.4e-7 (fp16-128 dec0) / 1.9e-7
(fp16-56 enc1.0); encoder chain 3.0e-4 (fp16-5 enc3.1); decoder chain 2.1e-4 / 2.1e-4 (the chains sit at the fp16 rounding of the
stored dv, 2^-11 / sqrt(3)).  Over (A)-(D) alone these were 1.8e-8 / 9.7e-8, 4.5e-4, 4.4e-4 / 3.8e-2, 2.2e-7 / 1.4e-7, 3.0e-4,
2.1e-4 / 2.1e-4: no new batch size moves a figure by more than a rounding.  The correct code exceeds none of the starting bounds, so
none was re-derived.  With the row count taken from the fp16 kernel's choice (the bug this file found), (B) and (D) gave rstd off by
45-60 % and the mean by up to 0.13 max(1, std) on enc1.1 / enc1.2 (and enc2.1 / enc2.2 in (D)), every other layer as above.
"""
import ctypes as C
import functools
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import vae_ref as R
from tests import test_vae_plan_cover as cover

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATENT = cover.LATENT
# name: (batch, operand mode, LO_HALO).  The default-knob configurations are cover.INSITU_BATCHES, which tests/test_vae_plan_cover.py
# proves to launch every layer in every way batch 1..128 does; (A) and (B) are its batch 64
CONFIGS = {"A": (64, "fp16", None), "B": (64, "fp8", None), "C": (2, "fp16", "3"), "D": (2, "fp8", "3")}
CONFIGS.update({f"{mode}-{b}": (b, mode, None) for mode in ("fp16", "fp8") for b in cover.INSITU_BATCHES[mode] if b != 64})
assert all(64 in cover.INSITU_BATCHES[mode] for mode in ("fp16", "fp8"))
ENC_CH = (3, 64, 128, 256, 512)
DEC_CH = (512, 256, 128, 64, 32)

# name: (bound, where it comes from)
BOUNDS = {
    "mean": (1e-4, "|dmean| / max(1, std): the partial sums' rtol"),
    "rstd": (1e-4, "|drstd| / rstd: the partial sums' rtol"),
    "output": (3e-3, "max abs / max(1, |y|max): test_gn_mish_forward_backward"),
    "conv": (4e-3, "max abs / max(1, |ref|max): test_conv_forward_and_gn_partials"),
    "conv_f8": (6e-2, "relative L2 per sample: tests/test_fp8_gpu.py"),
    "wgrad": (2e-4, "relative L2 over the sampled pairs: test_conv_wgrad"),
    "bgrad": (2e-4, "relative L2 over the layer's channels: as the weight gradient"),
    "dgrad": (3e-3, "relative L2 per tensor and sample: the op test's bound for dv"),
    "gn_bwd": (3e-3, "relative L2 per tensor and sample: test_gn_mish_forward_backward"),
}


def _layers():
    """The 16 conv + GroupNorm layers in forward order.  src / other name the stored tensors the layer reads."""
    out = []
    for s in range(4):
        p = f"encoder.down{s + 1}"
        for k, (conv, gn) in enumerate(((p + ".0", p + ".1"), (p + ".3.conv1.0", p + ".3.conv1.1"), (p + ".3.conv2.0", p + ".3.conv2.1"))):
            out.append(dict(name=f"enc{s}.{k}", dec=0, s=s, k=k, conv=conv, gn=gn, kind="s2" if k == 0 else "s1",
                            cin=ENC_CH[s] if k == 0 else ENC_CH[s + 1], cout=ENC_CH[s + 1],
                            src=("x" if s == 0 else f"enc{s - 1}.2/y") if k == 0 else f"enc{s}.{k - 1}/y",
                            mode=2 if k == 2 else 0, other=f"enc{s}.0/y" if k == 2 else None))
    for s in range(4):
        p = f"decoder.up{s + 1}"
        out.append(dict(name=f"dec{s}", dec=1, s=s, k=0, conv=p + ".0", gn=p + ".1", kind="t4", cin=DEC_CH[s], cout=DEC_CH[s + 1],
                        src="h0" if s == 0 else f"dec{s - 1}/y", mode=1 if s < 3 else 0, other=f"enc{2 - s}.2/y" if s < 3 else None))
    return out


LAYERS = _layers()
BY_NAME = {l["name"]: l for l in LAYERS}


def _pairs(layer):
    """(cout, cin) channels of the sampled weight-gradient entries: the grid of 8 x 8 channels (21 x 3 for the first conv), fixed seed."""
    g = torch.Generator().manual_seed(20260 + LAYERS.index(layer))
    ci = torch.randperm(layer["cin"], generator=g)[:min(8, layer["cin"])].sort().values
    co = torch.randperm(layer["cout"], generator=g)[:64 // len(ci)].sort().values
    return co, ci


def _samples(B):
    """first, one odd interior, last (0, 37, 63 at batch 64); every sample below batch 4"""
    if B < 4:
        return list(range(B))
    i = (37 * B) // 64 | 1
    return [0, i if i < B - 1 else 1, B - 1]


# ---- one step, read back ------------------------------------------------------------------------------------------------------
def _capture(B, precision):
    """One forward + fused backward (VAEStepper, lr = 0) and every tensor the checks need, on the CPU: per-sample tensors for the
    checked samples, whole-batch tensors reduced to the sampled channels (fp16 as stored), the fp64 sum of every dv (torch, on the
    device), the conv parameter gradients, the plan."""
    from lunaris_orion_amd import _lib
    from lunaris_orion_amd.trainer import VAEStepper
    from lunaris_orion_amd.vae import LunarisCoreVAE
    m = LunarisCoreVAE(latent_dim=LATENT, mfma_precision=precision)
    m.load_state_dict(R.closed_form_params(LATENT, 0))
    m = m.to("cuda")
    x = R.normalise_sprites(R.closed_form_sprites(B))
    st = VAEStepper(m, lr=0.0, weight_decay=0.0, max_grad_norm=1e9)
    scale = float(m.loss_scale)                         # what this step's backward multiplies its seeds by
    st.step(x.cuda(), 0, R.closed_form_eps(B, LATENT, salt=0).cuda())
    torch.cuda.synchronize()
    eng = st._last_engine
    assert eng is not None and eng.batch == B
    S = _samples(B)

    def dbg(which, s=0, k=0):
        off, dims, eb = C.c_size_t(), (C.c_int * 4)(), C.c_int()
        _lib.check(_lib.lib.lo_vae_debug_tensor_ex(eng.handle, which, s, k, C.byref(off), dims, C.byref(eb)), "lo_vae_debug_tensor_ex")
        shape = tuple(dims)
        n = shape[0] * shape[1] * shape[2] * shape[3]
        dt = {2: torch.float16, 4: torch.float32}[eb.value]
        return eng.ws[off.value:off.value + n * eb.value].view(dt).view(shape)

    T = {"B": B, "samples": S, "scale": scale, "ws_bytes": int(_lib.lib.lo_vae_workspace_bytes(eng.handle)), "fp8_layers": int(eng.fp8_layers),
         "x": x[S].clone(), "h0": dbg(9)[S].cpu()}
    for k in range(3):
        T[f"skipg{k}"] = dbg(10, k)[S].cpu()
    full = {"x": x.cuda().permute(0, 2, 3, 1), "h0": dbg(9)}        # whole-batch NHWC views on the device
    for l in LAYERS:
        n, s, k = l["name"], l["s"], l["k"]
        info = (C.c_int * 4)()
        _lib.check(_lib.lib.lo_vae_layer_plan(eng.handle, l["dec"], s, k, info), "lo_vae_layer_plan")
        T[n + "/plan"] = list(info)
        ex = (C.c_int * cover.FIELDS)()
        _lib.check(_lib.lib.lo_vae_layer_plan_ex(eng.handle, l["dec"], s, k, ex, cover.FIELDS), "lo_vae_layer_plan_ex")
        T[n + "/sig"] = cover.describe(tuple(ex))
        v = dbg(1 if l["dec"] else 0, s, k)
        y = dbg(3, s) if l["dec"] else (dbg(2, s) if k == 2 else dbg(4, s, k))
        dv = dbg(8 if l["dec"] else 7, s, k)
        full[n + "/y"] = y
        T[n + "/v"], T[n + "/y"], T[n + "/dv"] = v[S].cpu(), y[S].cpu(), dv[S].cpu()
        T[n + "/stats"] = dbg(6 if l["dec"] else 5, s, k)[S].view(len(S), 8, 2).cpu()
        co, ci = _pairs(l)
        T[n + "/in_sel"] = full[l["src"]][..., ci.cuda()].contiguous().cpu()
        T[n + "/dv_sel"] = dv[..., co.cuda()].contiguous().cpu()
        T[n + "/dv_sum"] = dv.double().sum(dim=(0, 1, 2)).cpu()
    assert sum(T[l["name"] + "/plan"][0] for l in LAYERS) == T["fp8_layers"]
    grads = {k_: g for (k_, _p), g in zip(m.named_parameters(), st.parameter_grads())}
    for l in LAYERS:
        T[l["name"] + "/dw"] = grads[l["conv"] + ".weight"].detach().cpu().clone()
        T[l["name"] + "/db"] = grads[l["conv"] + ".bias"].detach().cpu().clone()
    assert int(eng.sync_fail.item()) == 0
    # the next configuration's model and workspace (4 GB at batch 128) take this one's place
    del full, grads, eng, st, m
    torch.cuda.empty_cache()
    return T


_CHILD = r"""
import sys, torch
sys.path.insert(0, {root!r})
from tests.test_vae_insitu_gpu import _capture
torch.save(_capture({B}, {precision!r}), sys.argv[1])
print("INSITU_CAPTURED")
"""


@functools.lru_cache(maxsize=None)
def _run(cfg, tmpdir):
    B, precision, halo = CONFIGS[cfg]
    if halo is None:
        return _capture(B, precision)
    f = os.path.join(tmpdir, f"insitu_{cfg}.pt")
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT, B=B, precision=precision), f], env=dict(os.environ, LO_HALO=halo),
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "INSITU_CAPTURED" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
    return torch.load(f)


@pytest.fixture(scope="module")
def tmpdir_module(tmp_path_factory):
    return str(tmp_path_factory.mktemp("insitu"))


@pytest.fixture(scope="module", params=list(CONFIGS))
def fwd(request, tmpdir_module):
    return request.param, _run(request.param, tmpdir_module)


@pytest.fixture(scope="module", params=[c for c, (_b, mode, _h) in CONFIGS.items() if mode == "fp16"])
def bwd(request, tmpdir_module):
    return request.param, _run(request.param, tmpdir_module)


@functools.lru_cache(maxsize=None)
def _params():
    return R.closed_form_params(LATENT, 0)


# ---- references (fp64, CPU) ---------------------------------------------------------------------------------------------------
def _nchw(t):
    """stored NHWC (fp16 / fp32) -> fp64 NCHW"""
    return t.permute(0, 3, 1, 2).double().contiguous()


def _h16w(w):
    return w.to(torch.float16).double()


def _gn_mish(l, v, other):
    """v, other: fp64 NCHW.  The layer's output in its mode: 0 mish(GN(v)); 1 ... + other; 2 mish(... + other)."""
    P = _params()
    y = F.mish(F.group_norm(v, 8, P[l["gn"] + ".weight"].double(), P[l["gn"] + ".bias"].double(), R.GN_EPS))
    if l["mode"] == 1:
        y = y + other
    elif l["mode"] == 2:
        y = F.mish(y + other)
    return y


def _conv(l, x):
    P = _params()
    w, b = _h16w(P[l["conv"] + ".weight"]), P[l["conv"] + ".bias"].double()
    if l["kind"] == "t4":
        return F.conv_transpose2d(x, w, b, stride=2, padding=1)
    return F.conv2d(x, w, b, stride=2 if l["kind"] == "s2" else 1, padding=1)


def _conv_input_grad(l, dv, in_hw):
    """gradient wrt the layer's input of its conv, from dv (fp64 NCHW)"""
    w = _h16w(_params()[l["conv"] + ".weight"])
    if l["kind"] == "t4":
        return F.conv2d(dv, w, None, stride=2, padding=1)
    stride = 2 if l["kind"] == "s2" else 1
    return torch.nn.grad.conv2d_input((dv.shape[0], l["cin"], in_hw, in_hw), w, dv, stride=stride, padding=1)


def _gn_mish_bwd(l, v, dy):
    """dv of mish(GN(v)) (modes 0 and 1 have the same one) for the upstream gradient dy, by autograd in fp64"""
    P = _params()
    v = v.clone().requires_grad_(True)
    y = F.mish(F.group_norm(v, 8, P[l["gn"] + ".weight"].double(), P[l["gn"] + ".bias"].double(), R.GN_EPS))
    (g,) = torch.autograd.grad(y, v, dy)
    return g


def _rel(a, b):
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


# ---- figures: {layer: worst value over the checked samples} ---------------------------------------------------------------------
def stats_figures(T):
    out = {}
    for l in LAYERS:
        v = _nchw(T[l["name"] + "/v"])
        n, c = v.shape[0], v.shape[1]
        g = v.view(n, 8, -1)
        mean, var = g.mean(dim=2), g.var(dim=2, unbiased=False)
        rstd = 1.0 / torch.sqrt(var + R.GN_EPS)
        st = T[l["name"] + "/stats"].double()
        dm = ((st[:, :, 0] - mean).abs() / var.sqrt().clamp(min=1.0)).max().item()
        dr = ((st[:, :, 1] - rstd).abs() / rstd).max().item()
        out[l["name"]] = (dm, dr)
    return out


def output_figures(T):
    out = {}
    for l in LAYERS:
        other = _nchw(T[l["other"]]) if l["other"] else None
        ref = _gn_mish(l, _nchw(T[l["name"] + "/v"]), other)
        got = _nchw(T[l["name"] + "/y"])
        out[l["name"]] = max(((got[i] - ref[i]).abs().max() / max(1.0, ref[i].abs().max().item())).item() for i in range(ref.shape[0]))
    return out


def conv_figures(T):
    """{layer: (max abs error / max(1, |ref|max), relative L2), worst sample}; the first conv is not among them (its input is fp32,
    its kernel has an op test at its only shape)"""
    out = {}
    for l in LAYERS[1:]:
        ref = _conv(l, _nchw(T[l["src"]]))
        got = _nchw(T[l["name"] + "/v"])
        out[l["name"]] = (max(((got[i] - ref[i]).abs().max() / max(1.0, ref[i].abs().max().item())).item() for i in range(ref.shape[0])),
                          max(_rel(got[i], ref[i]) for i in range(ref.shape[0])))
    return out


def wgrad_figures(T):
    """{layer: (relative L2 of the sampled weight-gradient entries, relative L2 of the bias gradient)}"""
    out = {}
    for l in LAYERS:
        n = l["name"]
        co, ci = _pairs(l)
        x = _nchw(T[n + "/in_sel"]) if l["src"] != "x" else R.normalise_sprites(R.closed_form_sprites(T["B"])).double()[:, ci]
        dv = _nchw(T[n + "/dv_sel"]) / T["scale"]
        if l["kind"] == "t4":
            w = torch.zeros(len(ci), len(co), 4, 4, dtype=torch.float64, requires_grad=True)
            y = F.conv_transpose2d(x, w, None, stride=2, padding=1)
            got = T[n + "/dw"][ci][:, co].double()
        else:
            w = torch.zeros(len(co), len(ci), 3, 3, dtype=torch.float64, requires_grad=True)
            y = F.conv2d(x, w, None, stride=2 if l["kind"] == "s2" else 1, padding=1)
            got = T[n + "/dw"][co][:, ci].double()
        (ref,) = torch.autograd.grad(y, w, dv)
        out[n] = (_rel(got, ref), _rel(T[n + "/db"].double(), T[n + "/dv_sum"] / T["scale"]))
    return out


def encoder_chain_figures(T):
    """{enc{s}.1: relative L2 of dv against GroupNorm + Mish backward of the stored v seeded with conv2's data gradient, worst sample}"""
    out = {}
    for s in range(4):
        l1, l2 = BY_NAME[f"enc{s}.1"], BY_NAME[f"enc{s}.2"]
        v1 = _nchw(T[l1["name"] + "/v"])
        du = _conv_input_grad(l2, _nchw(T[l2["name"] + "/dv"]), v1.shape[2])
        ref = _gn_mish_bwd(l1, v1, du)
        got = _nchw(T[l1["name"] + "/dv"])
        out[l1["name"]] = max(_rel(got[i], ref[i]) for i in range(ref.shape[0]))
    return out


def decoder_chain_figures(T):
    """{dec{s}: (skip gradient 3-s against the transposed conv's input gradient of dec[s].dv, dec[s-1].dv against the GroupNorm + Mish
    backward seeded with the STORED skip gradient), worst sample}, s = 1..3"""
    out = {}
    for s in range(1, 4):
        l, lp = BY_NAME[f"dec{s}"], BY_NAME[f"dec{s - 1}"]
        skg = _nchw(T[f"skipg{3 - s}"])
        ref_g = _conv_input_grad(l, _nchw(T[l["name"] + "/dv"]), skg.shape[2])
        ref_dv = _gn_mish_bwd(lp, _nchw(T[lp["name"] + "/v"]), skg)
        got_dv = _nchw(T[lp["name"] + "/dv"])
        out[l["name"]] = (max(_rel(skg[i], ref_g[i]) for i in range(skg.shape[0])), max(_rel(got_dv[i], ref_dv[i]) for i in range(skg.shape[0])))
    return out


def _report(cfg, what, figs, T):
    """every layer's figure with the kernels and tiles it belongs to (lo_vae_layer_plan_ex)"""
    print(f"[insitu {cfg}] batch {T['B']} {what}:")
    for k, v in figs.items():
        print(f"[insitu {cfg}]   {k}={v if isinstance(v, float) else tuple(v)}  {T[k + '/sig']}")


def _named(bad, T):
    return {k: (v, T[k + "/sig"]) for k, v in bad.items()}


# ---- forward, every configuration -------------------------------------------------------------------------------------------
def test_groupnorm_statistics_match_the_stored_conv_output(fwd):
    cfg, T = fwd
    figs = stats_figures(T)
    _report(cfg, "statistics (dmean / max(1, std), drstd / rstd)", figs, T)
    bad = {k: v for k, v in figs.items() if not (v[0] <= BOUNDS["mean"][0] and v[1] <= BOUNDS["rstd"][0])}
    assert not bad, (cfg, _named(bad, T))


def test_layer_output_matches_groupnorm_mish_of_the_stored_conv_output(fwd):
    cfg, T = fwd
    figs = output_figures(T)
    _report(cfg, "output", figs, T)
    bad = {k: v for k, v in figs.items() if not v <= BOUNDS["output"][0]}
    assert not bad, (cfg, _named(bad, T))


def test_conv_output_matches_the_conv_of_the_stored_input(fwd):
    cfg, T = fwd
    figs = conv_figures(T)
    _report(cfg, "conv (max abs / max(1, |ref|max), relative L2)", figs, T)
    f8 = {l["name"] for l in LAYERS if T[l["name"] + "/plan"][0]}
    assert (len(f8) > 0) == (CONFIGS[cfg][1] == "fp8")
    bad = {k: v for k, v in figs.items() if not (v[1] <= BOUNDS["conv_f8"][0] if k in f8 else v[0] <= BOUNDS["conv"][0])}
    assert not bad, (cfg, _named(bad, T), sorted(f8))


# ---- backward, the fp16 configurations ------------------------------------------------------------------------------------------------------
def test_weight_and_bias_gradients_match_the_stored_operands(bwd):
    cfg, T = bwd
    figs = wgrad_figures(T)
    _report(cfg, "weight / bias gradient", figs, T)
    bad = {k: v for k, v in figs.items() if not (v[0] <= BOUNDS["wgrad"][0] and v[1] <= BOUNDS["bgrad"][0])}
    assert not bad, (cfg, _named(bad, T))


def test_encoder_data_gradient_and_groupnorm_backward_chain(bwd):
    cfg, T = bwd
    figs = encoder_chain_figures(T)
    _report(cfg, "encoder dgrad + GroupNorm backward", figs, T)
    bad = {k: v for k, v in figs.items() if not v <= BOUNDS["gn_bwd"][0]}
    assert not bad, (cfg, _named(bad, T))


def test_decoder_data_gradient_and_groupnorm_backward_chain(bwd):
    cfg, T = bwd
    figs = decoder_chain_figures(T)
    _report(cfg, "decoder skip gradient, GroupNorm backward", figs, T)
    bad = {k: v for k, v in figs.items() if not (v[0] <= BOUNDS["dgrad"][0] and v[1] <= BOUNDS["gn_bwd"][0])}
    assert not bad, (cfg, _named(bad, T))


# ---- the fp8 forward's partial-sum rows stay inside their buffer ------------------------------------------------------------------
_POISON_CHILD = r"""
import sys, pytest, torch
sys.path.insert(0, {root!r})
from tests import test_workspace_poison_gpu as W
mp = pytest.MonkeyPatch()
try:
    W._three_runs(mp, lambda: W._stepper_run(2, precision="fp8"))
finally:
    mp.undo()
print("POISON_FP8_HALO3_OK")
"""


def test_fp8_mode_on_poisoned_workspace_with_the_fused_tap_kernel_forced_on():
    """tests/test_workspace_poison_gpu.py's fp8 scenario at a shape where the e4m3 launch of a ResBlock conv used to write more
    partial-sum rows than the plan had room for (LO_HALO=3, batch 2): bitwise equal on zero / 0xFF / 0x7B workspaces, guards intact.
    LO_HALO is read once per process, hence the child."""
    r = subprocess.run([sys.executable, "-c", _POISON_CHILD.format(root=ROOT)], env=dict(os.environ, LO_HALO="3"), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "POISON_FP8_HALO3_OK" in r.stdout, r.stdout[-1500:] + r.stderr[-3000:]
