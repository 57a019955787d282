"""LunarMoETeacher on MI355X: the reference's ``nn.Module`` surface, forward in liblunaris_hip.so.

Drop-in contract (reference: /root/reference/lunar_evaluator.py:278-462): same constructor signature, the same 252
parameters + 99 buffers under the same ``state_dict`` keys (``feature_extractor.conv1.0.weight`` ...
``prompt_net.6.bias``; BatchNorm ``running_mean/var/num_batches_tracked``; the attention buffer
``last_spatial_shapes``), the reference's initialisation (``kaiming_normal_(fan_out, leaky_relu)``, zero biases,
unit norms, ``rel_pos ~ N(0, 0.02)``, ``layer_scale = 0.1``), ``forward(x, prompt_embedding=None)`` returning the same
six-key dict.  The sub-modules are containers; ``forward`` is one native call (``lo_teacher_forward``) that reproduces
the forward AS EXECUTED — including the chunk-index write offset of ``PixelArtAttention``.

Dropout (``dropout_rate``, default 0.1 like the reference; lunar_evaluator.py:97-99,139-140,212,225,246,253,353-397): in
train mode all six sites are applied on the device with torch semantics (``nn.Dropout`` elementwise, ``nn.Dropout2d`` per
(sample, channel), kept values scaled by 1/(1-p)).  The masks come from a counter RNG keyed by (torch seed, rank, call,
site, element) — ``oracle/dropout_ref.py`` regenerates them bit-exactly, which is how the parity tests run the CPU oracle
and the reference itself on the same masks.  With dropout the native forward runs every 3x3 convolution in full (the
constant-field shortcuts of the p = 0 path do not survive ``proj_drop``); eval mode and ``dropout_rate=0`` take the
shortcut path.  ``quality_scores`` and ``expert_weights`` are autograd-visible outputs: with gradients enabled the forward is an
autograd node over the gate / quality-head parameters — the only ones that receive gradients in the reference, whose reentrant
checkpoints cut the experts and the feature extractor from the graph — so the reference's own
``teacher_loss.backward()`` (train_hybrid.py:891-904) fills their ``.grad`` (``lo_teacher_heads_backward_ex``, replaying the
call's dropout masks).  ``trainer.HybridStepper`` takes the same gradients in coefficient form (``heads_backward``).  In-place
parameter updates by any optimizer are noticed through the parameters' version counters (re-pack before the next forward).

``feature_dim``: 128 (the CLI default: folded attention + constant-field shortcuts when no dropout is active) or 256 / 512 (the
README's High-End recipe, /root/reference/README.md:102-118: a generic path with every tensor at full resolution and the
``ExpertBlock.shortcut`` Conv1x1 + BatchNorm of the first block, lunar_evaluator.py:254-257).  ``feature_maps`` is always ``None``.

``mfma_precision="fp8"`` (any ``feature_dim``): the 24 full-resolution 3x3 convolutions of a train-mode forward take OCP e4m3
operands (fp16 outputs, fp32 BatchNorm statistics); at 256 / 512 these are the 128 -> F and F -> F implicit-GEMM launches that
carry nearly all of the teacher's time.  Eval mode stays fp16, bit for bit.
"""
from __future__ import annotations

import ctypes as C
import warnings
from typing import Dict, NamedTuple, Optional

import torch
import torch.nn as nn

from . import _lib


class PixelArtFeatureExtractor(nn.Module):
    """Parameter container (lunar_evaluator.py:57-112)."""

    def __init__(self, in_channels=3, dropout_rate=0.1, feature_dim=128):
        super().__init__()
        self.conv1 = nn.Sequential(nn.Conv2d(in_channels, 32, 3, padding=1), nn.LeakyReLU(0.2), nn.BatchNorm2d(32))

        def branch(k):
            return nn.Sequential(nn.Conv2d(32, 32, k, padding=k // 2, groups=32), nn.Conv2d(32, 64, 1), nn.LeakyReLU(0.2), nn.BatchNorm2d(64))
        self.edge_branch, self.color_branch, self.detail_branch = branch(3), branch(5), branch(3)
        self.dropout = nn.Dropout(dropout_rate)
        self.fusion = nn.Sequential(nn.Conv2d(192, feature_dim, 1), nn.LeakyReLU(0.2), nn.BatchNorm2d(feature_dim))


class PixelArtAttention(nn.Module):
    """Parameter container (lunar_evaluator.py:119-144)."""

    def __init__(self, in_channels, num_heads=8, rel_pos_size=8, dropout=0.1, chunk_size=64):
        super().__init__()
        self.num_heads, self.head_dim, self.chunk_size = num_heads, in_channels // num_heads, chunk_size
        self.qkv = nn.Conv2d(in_channels, in_channels * 3, 1)
        self.proj = nn.Conv2d(in_channels, in_channels, 1)
        self.rel_pos_h = nn.Parameter(torch.randn(1, num_heads, rel_pos_size, 1) * 0.02)
        self.rel_pos_w = nn.Parameter(torch.randn(1, num_heads, 1, rel_pos_size) * 0.02)
        self.attn_drop, self.proj_drop = nn.Dropout(dropout), nn.Dropout(dropout)
        self.register_buffer("rel_pos_cache", None)
        self.register_buffer("last_spatial_shapes", torch.zeros(2))


class ExpertBlock(nn.Module):
    """Parameter container (lunar_evaluator.py:234-258)."""

    def __init__(self, in_channels, out_channels, dropout_rate=0.1, rel_pos_size=8, layer_scale_init=0.1):
        super().__init__()
        def cb(ci):
            return nn.Sequential(nn.Conv2d(ci, out_channels, 3, padding=1), nn.LeakyReLU(0.2), nn.BatchNorm2d(out_channels), nn.Dropout2d(dropout_rate))
        self.conv1 = cb(in_channels)
        self.attention = PixelArtAttention(out_channels, rel_pos_size=rel_pos_size, dropout=dropout_rate)
        self.conv2 = cb(out_channels)
        self.shortcut = (nn.Sequential(nn.Conv2d(in_channels, out_channels, 1), nn.BatchNorm2d(out_channels))
                         if in_channels != out_channels else nn.Identity())
        self.layer_scale = nn.Parameter(torch.ones(1, out_channels, 1, 1) * layer_scale_init)


# gscale of lo_teacher_eval_backward (the train path passes 2**20).  Eval-mode activation gradients are smaller than train-mode ones
# (x.grad 57x in norm for the same loss on the closed-form state), so 2**20 was not taken for granted:
# tests/test_teacher_eval_grad_gpu.py::test_gscale_2p20_and_2p24 runs 2**20 and 2**24 against the fp16-rounding oracle.  Measured on the
# MI355X: both 4.168e-3 from it (16x16-pooled 8.5e-4) and 5.8e-5 from each other -- no underflow at 2**20, which keeps 16x more
# headroom below fp16's maximum for larger upstream gradients, so the train path's value stays.
EVAL_GSCALE = 2 ** 20
TRAIN_GSCALE = 2 ** 20          # gscale of lo_teacher_full_backward_dx: upstream gradients of order 1 (normalised on the device first)


def loss_gscale(B: int) -> float:
    """gscale of the coefficient-form backward (upstream = coef / (4 B) per element): a power of two for power-of-two batches; any
    positive value is exact enough."""
    return 64.0 * B * 16384.0


def _call(name: str, *args) -> None:
    """One checked call of a library entry point, named once."""
    _lib.check(getattr(_lib.lib, name)(*args), name)


def _alloc_workspace(nbytes: int, device: torch.device) -> torch.Tensor:
    """Device memory for a teacher engine's workspace (`ws`), full-backward scratch (`bws`) or head-gradient `rows`; contents unspecified, see
    `vae._alloc_workspace`.  The poisoned-workspace tests swap this function."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


class TeacherRoute(NamedTuple):
    backward: str       # "heads" | "train_full" | "eval_full": which native backward the call's autograd node takes
    want_dx: bool       # the images get their gradient
    live_set: str       # "heads" (gate.*, quality_heads.*) | "path" (all but semantic_head, style_net, prompt_net)
    warn: bool          # eval mode without eval_input_grad: the input requires grad and gets none


def teacher_route(training: bool, eval_input_grad: bool, all_parameters_live: bool, x_requires_grad: bool) -> TeacherRoute:
    """The one decision of `LunarMoETeacher.forward` (its docstring has the table); pure, no tensors."""
    if not training and not eval_input_grad:
        return TeacherRoute("heads", False, "path" if all_parameters_live else "heads", bool(x_requires_grad))
    if not (all_parameters_live or x_requires_grad):
        return TeacherRoute("heads", False, "heads", False)
    return TeacherRoute("train_full" if training else "eval_full", bool(x_requires_grad), "path", False)


class _TeacherEngine:
    """Native plan + everything that is per batch size: the workspace, the full-backward scratch, the head-gradient rows and the engine's
    constants (head gradient range, where a forward leaves the heads' inputs).  The handle is released with the object (lo_teacher_destroy)."""

    def __init__(self, model: "LunarMoETeacher", batch: int):
        h = C.c_void_p()
        _lib.check(_lib.lib.lo_teacher_create_ex(batch, model.num_experts, model.feature_dim, model.embedding_dim,
                                                 1 if model.mfma_precision == "fp8" else 0, C.byref(h)), "lo_teacher_create_ex")
        self.handle, self.batch = h, batch
        self.ws = _alloc_workspace(_lib.lib.lo_teacher_workspace_bytes(h), model._flat.device)
        self.bws: Optional[torch.Tensor] = None
        self._rows: Optional[torch.Tensor] = None
        self.packed_version = None
        b, e = C.c_size_t(), C.c_size_t()
        _call("lo_teacher_grad_range", h, C.byref(b), C.byref(e))
        self.heads_range = (b.value, e.value)
        offs, elems = (C.c_size_t * 3)(), (C.c_size_t * 3)()
        _call("lo_teacher_heads_saved", h, offs, elems)
        self.saved_offsets, self.saved_elems = tuple(int(o) for o in offs), tuple(int(n) for n in elems)
        self._saved = tuple(self.ws[o:o + 4 * n].view(torch.float32) for o, n in zip(self.saved_offsets, self.saved_elems))

    def backward_scratch(self) -> torch.Tensor:
        """`bws` of the kept forwards and the full backwards (26 GB at batch 64, feature_dim 128), made on first use."""
        if self.bws is None:
            self.bws = _alloc_workspace(_lib.lib.lo_teacher_full_backward_bytes(self.handle), self.ws.device)
        return self.bws

    def rows(self) -> torch.Tensor:
        """The [B][heads range] fp32 scratch of every backward's head part, made on first use."""
        if self._rows is None:
            self._rows = _alloc_workspace(self.batch * (self.heads_range[1] - self.heads_range[0]) * 4, self.ws.device).view(torch.float32)
        return self._rows

    def saved_views(self):
        """Where a forward leaves the heads' inputs in `ws`: pooled features, pooled expert features, pre-weighting logits."""
        return self._saved

    def __del__(self):
        h, self.handle = getattr(self, "handle", None), None
        if h is not None:
            try:
                _lib.lib.lo_teacher_destroy(h)
            except Exception:
                pass


class _TeacherFunction(torch.autograd.Function):
    """LunarMoETeacher.forward as an autograd node (lunar_evaluator.py:353-373, 417, 431-432): differentiable outputs quality_scores
    [B,4] and expert_weights [B,E]; the embeddings and the semantic score are returned without a graph (nothing in the reference
    step differentiates them).  The `TeacherRoute` it is given names the forward it runs and the backward it takes.  The head inputs
    of THIS call (pooled features, pre-weighting logits, dropout stream) are copied out of the workspace, so later forward calls do
    not disturb it."""
    FORWARD_MODE = {"heads": "auto", "train_full": "keep", "eval_full": "keep_eval"}

    @staticmethod
    def forward(ctx, model, route, x, *live):
        xd = x.detach().contiguous().float()
        out, eng, p, seed = model._native_forward(xd, mode=_TeacherFunction.FORWARD_MODE[route.backward])
        ctx.route, ctx.x, ctx.x_dtype = route, (xd if route.backward != "heads" else None), x.dtype
        ctx.model, ctx.eng, ctx.drop = model, eng, (p, seed)
        ctx.live_offsets = [(t.data_ptr() - model._flat.data_ptr()) // 4 for t in live]
        ctx.live_shapes = [t.shape for t in live]
        ctx.save_for_backward(out["expert_weights"], *(v.clone() for v in eng.saved_views()))
        ctx.mark_non_differentiable(out["style_embedding"], out["prompt_embedding"], out["semantic_score"])
        return out["quality_scores"], out["expert_weights"], out["style_embedding"], out["prompt_embedding"], out["semantic_score"]

    @staticmethod
    def backward(ctx, gq, gw, *_):
        model, route = ctx.model, ctx.route
        w, *saved = ctx.saved_tensors
        cont = lambda t: None if t is None else t.contiguous().float()
        gq, gw = cont(gq), cont(gw)
        full = route.backward != "heads"
        # (the eval backward with no live parameter computes no parameter gradient: its flat buffer is NULL)
        grads = torch.zeros_like(model._flat) if (ctx.live_offsets or route.backward != "eval_full") else None
        dx = torch.empty_like(ctx.x) if full and route.want_dx and ctx.needs_input_grad[2] and (gq is not None or gw is not None) else None
        if (gq is not None or gw is not None) and (grads is not None or dx is not None):
            scr = None
            if full:
                # a foreign loss scale (GradScaler: 65 536) is divided out on the device first, like at the VAE's boundary, so that the
                # fp16 activation gradients see upstream values of order 1
                from .vae import _normalise_upstream
                scr, (gq, gw) = _normalise_upstream([gq, gw])
            model._native_backward(ctx.eng, route.backward, ctx.x, saved, w, gq, gw, ctx.drop, grads, dx)
            for t in (grads, dx):
                if scr is not None and t is not None:
                    _call("lo_grad_unscale_dev", t.data_ptr(), t.numel(), scr.data_ptr() + 4, None, _lib.stream_ptr())
        if dx is not None and ctx.x_dtype != torch.float32:
            dx = dx.to(ctx.x_dtype)
        return (None, None, dx) + tuple(grads[o:o + shape.numel()].view(shape) for o, shape in zip(ctx.live_offsets, ctx.live_shapes))


class LunarMoETeacher(nn.Module):
    def __init__(self, num_experts=4, feature_dim=128, dropout_rate=0.1, rel_pos_size=8, use_checkpointing=True,
                 expert_layers=3, intermediate_dim=256, embedding_dim=64, mfma_precision: str = "fp16", full_backward: bool = False,
                 eval_input_grad: bool = False):
        super().__init__()
        # eval_input_grad (an addition of this build, opt-in): in eval mode an input that requires grad gets its gradient (and, with
        # full_backward, the trunk its parameter gradients) through BatchNorm at the running statistics -- see `forward`.  Default:
        # the eval-mode teacher gives the images no gradient and warns
        self.eval_input_grad = bool(eval_input_grad)
        # full_backward (an addition of this build): the autograd graph of `quality_scores` / `expert_weights` covers EVERY
        # parameter on their path -- experts and feature extractor included -- i.e. the reference with `use_reentrant=False` at its three
        # checkpoint calls (lunar_evaluator.py:194-197, 266-275, 411-414).  Default: the reference as it executes (gate + quality heads only).
        self.all_parameters_live = bool(full_backward)
        # mfma_precision (an addition of this build): "fp16" (default, parity-tested) or "fp8" = OCP e4m3 operands in the 24
        # full-resolution 3x3 convolutions of a train-mode forward (BASELINE config 5) -- feature_dim 128: on the dropout path
        # (dropout_rate > 0); 256 / 512: in every train-mode forward, the statistics-only one included.  Eval mode, the kept forward
        # of the full backward and every backward are fp16 either way
        if mfma_precision not in ("fp16", "fp8"):
            raise ValueError(f"mfma_precision must be 'fp16' or 'fp8', got {mfma_precision!r}")
        self.mfma_precision = mfma_precision
        if feature_dim not in (128, 256, 512) or expert_layers != 3 or intermediate_dim != 256 or rel_pos_size != 8:
            raise NotImplementedError("built: feature_dim 128 (the CLI default), 256 or 512 (README High-End recipe) with expert_layers=3, "
                                      "intermediate_dim=256, rel_pos_size=8 (the CLI defaults)")
        self.num_experts, self.feature_dim, self.dropout_rate = num_experts, feature_dim, dropout_rate
        self.rel_pos_size, self.use_checkpointing, self.expert_layers = rel_pos_size, use_checkpointing, expert_layers
        self.intermediate_dim, self.embedding_dim = intermediate_dim, embedding_dim
        self.feature_extractor = PixelArtFeatureExtractor(3, dropout_rate, 128)

        def expert():
            blocks, cin = [], 128
            for _ in range(expert_layers):
                blocks.append(ExpertBlock(cin, feature_dim, dropout_rate, rel_pos_size))
                cin = feature_dim
            return nn.Sequential(*blocks)
        self.experts = nn.ModuleList([expert() for _ in range(num_experts)])
        self.gate = nn.Sequential(nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.Linear(128, intermediate_dim), nn.LeakyReLU(0.2),
                                  nn.Dropout(dropout_rate), nn.Linear(intermediate_dim, num_experts), nn.Softmax(dim=1))

        def head(hidden, out, sigmoid=False):
            mods = [nn.AdaptiveAvgPool2d(1), nn.Flatten(), nn.LayerNorm(feature_dim), nn.Linear(feature_dim, hidden), nn.LeakyReLU(0.2),
                    nn.Dropout(dropout_rate), nn.Linear(hidden, out)]
            return nn.Sequential(*(mods + ([nn.Sigmoid()] if sigmoid else [])))
        self.quality_heads = nn.ModuleList([head(intermediate_dim // 4, 4) for _ in range(num_experts)])
        self.semantic_head = head(intermediate_dim // 2, 1, sigmoid=True)
        self.style_net = head(intermediate_dim // 2, embedding_dim)
        self.prompt_net = head(intermediate_dim // 2, embedding_dim)
        self.apply(self._init_weights)
        self._flat: Optional[torch.Tensor] = None
        self._nbt: Optional[torch.Tensor] = None      # the BatchNorm step counters, stacked (see _ensure_flat)
        self._engines: Dict[int, "_TeacherEngine"] = {}
        self._weights_version = 0
        self._drop_seed: Optional[int] = None     # counter-RNG stream of the dropout masks; derived at the first train-mode forward
        self._drop_exact = False                   # set_dropout_stream(exact_next=True): the next call seed is the stream seed itself
        self.drop_calls = 0                        # train-mode forwards drawn from the stream so far (checkpointed)
        self.last_drop_seed: Optional[int] = None  # the seed the last forward ran with (tests regenerate its masks from it)

    @staticmethod
    def _init_weights(m):
        """lunar_evaluator.py:399-406."""
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="leaky_relu")
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, (nn.BatchNorm2d, nn.LayerNorm)):
            nn.init.ones_(m.weight)
            nn.init.zeros_(m.bias)

    # ---- flat state ---------------------------------------------------------------------------------------
    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        self._flat = None
        self._engines.clear()
        return out

    def load_state_dict(self, *a, **kw):
        out = super().load_state_dict(*a, **kw)
        self._weights_version += 1
        return out

    def mark_weights_changed(self):
        self._weights_version += 1

    def _named_state(self):
        params = dict(self.named_parameters())
        bufs = dict(self.named_buffers())
        for k in self.state_dict().keys():
            yield k, (params[k] if k in params else bufs[k])

    def _ensure_flat(self):
        first = next(self.parameters())
        if (self._flat is not None and self._flat.device == first.device
                and self._flat.data_ptr() <= first.data_ptr() < self._flat.data_ptr() + 4 * self._flat.numel()):
            return
        _lib.require_gpu()
        if first.device.type != "cuda":
            raise _lib.LunarisHipError("LunarMoETeacher must be on the GPU (model.to('cuda')); there is no CPU path")
        h = C.c_void_p()
        _lib.check(_lib.lib.lo_teacher_create(1, self.num_experts, self.feature_dim, self.embedding_dim, C.byref(h)), "lo_teacher_create")
        try:
            state = list(self._named_state())
            assert _lib.lib.lo_teacher_num_tensors(h) == len(state), "teacher state table size mismatch"
            flat = torch.zeros(_lib.lib.lo_teacher_flat_elems(h), dtype=torch.float32, device=first.device)
            with torch.no_grad():
                for i, (k, t) in enumerate(state):
                    assert _lib.lib.lo_teacher_tensor_name(h, i).decode() == k, (i, k)
                    assert _lib.lib.lo_teacher_tensor_numel(h, i) == t.numel(), k
                    off = _lib.lib.lo_teacher_tensor_offset(h, i)
                    if off < 0:
                        continue                      # integer buffer (num_batches_tracked) stays a normal tensor
                    flat[off:off + t.numel()].copy_(t.detach().reshape(-1).float())
                    t.data = flat[off:off + t.numel()].view(t.shape)
        finally:
            _lib.lib.lo_teacher_destroy(h)
        # the 29 BatchNorm step counters become views of ONE int64 tensor: a train-mode forward bumps them with one launch
        # (29 separate `num_batches_tracked += 1` cost 29 launches = 0.13 ms of GPU time and more of host time per forward)
        bns = [m for m in self.modules() if isinstance(m, nn.BatchNorm2d)]
        with torch.no_grad():
            nbt = torch.stack([m.num_batches_tracked.detach().reshape(()).to(first.device, torch.int64) for m in bns])
            for i, m in enumerate(bns):
                m.num_batches_tracked.data = nbt[i]
        self._nbt = nbt
        self._flat = flat
        self._weights_version += 1
        self._engines.clear()

    def _engine(self, batch: int):
        self._ensure_flat()
        eng = self._engines.get(batch)
        if eng is None:
            eng = _TeacherEngine(self, batch)
            self._engines[batch] = eng
        # in-place updates by any optimizer move the parameters' version counters (the native head update writes through raw
        # pointers instead and touches only tensors the head kernels read in fp32: nothing to re-pack)
        version = (self._weights_version, sum(p._version for p in self.parameters()))
        if eng.packed_version != version:
            _lib.check(_lib.lib.lo_teacher_pack(eng.handle, self._flat.data_ptr(), eng.ws.data_ptr(), _lib.stream_ptr()), "lo_teacher_pack")
            eng.packed_version = version
        return eng

    def live_parameters(self):
        """The parameters that receive gradients in the reference step (gate.*, quality_heads.*: SURVEY §3.2), state_dict order; with
        ``LunarMoETeacher(full_backward=True)`` every parameter on the path of quality_scores / expert_weights (all but the style / prompt / semantic heads)."""
        return self._live_parameters("path" if self.all_parameters_live else "heads")

    def _live_parameters(self, live_set: str):
        if live_set == "path":
            return [p for k, p in self.named_parameters() if k.split(".")[0] not in ("semantic_head", "style_net", "prompt_net")]
        return [p for k, p in self.named_parameters() if k.startswith("gate.") or k.startswith("quality_heads.")]

    # ---- dropout stream -----------------------------------------------------------------------------------
    def set_dropout_stream(self, seed: int, exact_next: bool = False) -> None:
        """Restart the dropout mask stream from ``seed`` (otherwise derived from ``torch.initial_seed()`` and the rank).
        ``exact_next``: the next train-mode forward uses ``seed`` itself as its call seed (parity tests)."""
        self._drop_seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._drop_exact = bool(exact_next)

    def _next_drop_seed(self) -> int:
        """One 64-bit stream value per forward call (the same scheme as the VAE's noise stream, vae.py): keyed by the torch
        seed (`--seed`, train_hybrid.py:1138-1141) and the rank, advanced by an LCG per call."""
        if self._drop_seed is None:
            import torch.distributed as dist
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
            self._drop_seed = (torch.initial_seed() * 0x9E3779B97F4A7C15 + 0xD209 + 0xD1B54A32D192ED03 * rank) & 0xFFFFFFFFFFFFFFFF
            from .vae import lcg_advance
            self._drop_seed = lcg_advance(self._drop_seed, self.drop_calls)     # > 0 after a resume: same stream, same position
        if self._drop_exact:
            self._drop_exact = False
        else:
            self._drop_seed = (self._drop_seed * 6364136223846793005 + 1442695040888963407) & 0xFFFFFFFFFFFFFFFF
            self.drop_calls += 1
        self.last_drop_seed = self._drop_seed
        return self._drop_seed

    def last_path(self, batch: int) -> int:
        """0 = sparse shortcuts, 1 = dense (LO_T_DENSE=1), 2 = dropout path; -1 before the first forward of that batch size."""
        eng = self._engines.get(batch)
        return -1 if eng is None else int(_lib.lib.lo_teacher_last_path(eng.handle))

    def update_statistics_only(self, x: torch.Tensor) -> None:
        """The side effects of `forward(x)` in train mode without its outputs: every BatchNorm layer sees the batch
        (running statistics, `num_batches_tracked`), the pooling of the last ExpertBlocks and the heads are skipped.
        `_process_batch` calls the teacher once this way (train_hybrid.py:853-855: the result is overwritten unused)."""
        if self.training:
            self._native_forward(x, out=(None,) * 5)

    def _native_forward(self, x: torch.Tensor, mode: str = "auto", out=None, keep: bool = False):
        """The one call site of the three forwards.  mode "auto": `lo_teacher_forward` in the module's mode.  "keep" (spelled `keep=True`
        by older callers): `lo_teacher_forward_keep`, the train-mode forward of a step that ends in a full backward -- every block's
        output stays in the backward's scratch; on an eval-mode module it is "auto".  "keep_eval": `lo_teacher_forward_keep_eval`, the
        same for `lo_teacher_eval_backward`; it runs at the running statistics without dropout whatever the module's mode and moves
        no state (no BatchNorm counter, no dropout-seed draw).  out: caller-owned (quality_scores, expert_weights, style_embedding,
        prompt_embedding, semantic_score), None entries passed as NULL (skipped).  Returns (outputs, engine, dropout_p, call seed)."""
        if x.dim() != 4 or tuple(x.shape[1:]) != (3, 128, 128):
            raise ValueError(f"expected input of shape [B, 3, 128, 128], got {tuple(x.shape)}")
        x = x.detach().contiguous().float()
        B = x.shape[0]
        eng = self._engine(B)
        if out is None:
            out = tuple(torch.empty(B, n, dtype=torch.float32, device=x.device) for n in (4, self.num_experts, self.embedding_dim, self.embedding_dim, 1))
        outs = tuple(_lib.ptr(t) for t in out)
        head = (eng.handle, x.data_ptr(), self._flat.data_ptr(), eng.ws.data_ptr())
        if mode == "keep_eval":
            p, seed = 0.0, 0
            _call("lo_teacher_forward_keep_eval", *head, eng.backward_scratch().data_ptr(), *outs, _lib.stream_ptr())
        else:
            p = float(self.dropout_rate) if self.training else 0.0
            seed = self._next_drop_seed() if p > 0 else 0
            if (keep or mode == "keep") and self.training:
                _call("lo_teacher_forward_keep", *head, eng.backward_scratch().data_ptr(), p, seed, *outs, _lib.stream_ptr())
            else:
                _call("lo_teacher_forward", *head, 1 if self.training else 0, p, seed, *outs, _lib.stream_ptr())
            if self.training:
                with torch.no_grad():
                    self._nbt += 1
        q, w, st, pr, sem = out
        return ({"quality_scores": q, "expert_weights": w, "style_embedding": st, "prompt_embedding": pr, "semantic_score": sem, "feature_maps": None}, eng, p, seed)

    def _native_backward(self, eng, backward: str, x, saved, weights, gq, gw, drop, grads, dx, seed=None) -> None:
        """The one call site of the four backwards that take upstream gradients gq [B,4] / gw [B,E] (either may be None).  backward: a
        `TeacherRoute.backward`; saved: the forward's three head inputs (`eng.saved_views()` or clones of them); drop: the forward's
        (dropout_p, call seed); grads: flat gradient in the layout of `_flat`, or None (eval_full: no parameter gradient is computed);
        dx: the images' gradient or None.  seed = (target, coef, factor), eval_full only: `lo_teacher_eval_backward_seed`, whose last
        kernel stores factor * dx + coef[0] * (x - target) into dx."""
        heads = tuple(t.data_ptr() for t in saved) + (weights.data_ptr(), _lib.ptr(gq), _lib.ptr(gw))
        rows, st = eng.rows().data_ptr(), _lib.stream_ptr()
        if backward == "heads":
            _call("lo_teacher_heads_backward_ex", eng.handle, self._flat.data_ptr(), *heads, float(drop[0]), int(drop[1]), rows, grads.data_ptr(), st)
            return
        trunk = (eng.handle, x.data_ptr(), self._flat.data_ptr(), eng.ws.data_ptr(), eng.backward_scratch().data_ptr()) + heads
        if backward == "train_full":
            _call("lo_teacher_full_backward_dx", *trunk, float(drop[0]), int(drop[1]), float(TRAIN_GSCALE), rows, grads.data_ptr(), _lib.ptr(dx), st)
        elif seed is None:
            _call("lo_teacher_eval_backward", *trunk, float(EVAL_GSCALE), rows, _lib.ptr(grads), _lib.ptr(dx), st)
        else:
            target, coef, factor = seed
            _call("lo_teacher_eval_backward_seed", *trunk, float(EVAL_GSCALE), rows, target.data_ptr(), coef.data_ptr(), float(factor), dx.data_ptr(), st)

    def full_backward(self, x: torch.Tensor, expert_weights: torch.Tensor, coef: float, gscale: float = None, out: torch.Tensor = None) -> torch.Tensor:
        """SURVEY §8 row F2, second half: gradients of ``coef * -mean(quality_scores)`` (train_hybrid.py:891-892, coef =
        quality_weight / accumulation steps) for EVERY teacher parameter on the loss path -- what ``teacher_loss.backward()``
        yields when the model's three ``checkpoint`` calls (lunar_evaluator.py:194-197, 266-275, 411-414) are non-reentrant.
        Must follow the train-mode ``forward(x)`` whose loss it differentiates (same images; the call's dropout stream and head
        inputs are replayed).  Returns the flat gradient in the layout of ``self._flat`` (``parameter_grad_views`` slices it); with
        ``out`` it is written there and nothing is allocated."""
        x = x.detach().contiguous().float()
        eng = self._engine(x.shape[0])
        grads = torch.empty_like(self._flat) if out is None else out
        _call("lo_teacher_full_backward", eng.handle, x.data_ptr(), self._flat.data_ptr(), eng.ws.data_ptr(), eng.backward_scratch().data_ptr(),
              expert_weights.contiguous().float().data_ptr(), float(coef), float(loss_gscale(x.shape[0]) if gscale is None else gscale),
              eng.rows().data_ptr(), grads.data_ptr(), _lib.stream_ptr())
        return grads

    def heads_backward(self, expert_weights: torch.Tensor, coef: float, out: torch.Tensor) -> torch.Tensor:
        """The same loss for the gate and the quality heads only, the parameters the reference step trains (lo_teacher_heads_backward:
        reads what the last forward of this batch size left in the workspace), into the head range of ``out``."""
        eng = self._engine(expert_weights.shape[0])
        _call("lo_teacher_heads_backward", eng.handle, self._flat.data_ptr(), eng.ws.data_ptr(), expert_weights.data_ptr(), float(coef),
              eng.rows().data_ptr(), out.data_ptr(), _lib.stream_ptr())
        return out

    def parameter_grad_views(self, flat_grads: torch.Tensor):
        """name -> view of ``flat_grads`` (layout of ``self._flat``) for every parameter."""
        base = self._flat.data_ptr()
        return {k: flat_grads[(p.data_ptr() - base) // 4:(p.data_ptr() - base) // 4 + p.numel()].view(p.shape) for k, p in self.named_parameters()}

    def forward(self, x: torch.Tensor, prompt_embedding=None):
        """lunar_evaluator.py:408-462.  ``prompt_embedding`` is accepted and ignored exactly like the reference does
        (it is overwritten at :438 before any use).  With gradients enabled, ``quality_scores`` / ``expert_weights`` carry a graph
        (`_TeacherFunction`) whose backward `teacher_route` picks; ``full`` = the constructor's ``full_backward``, ``x_rg`` = the input
        requires grad (the teacher as a differentiable reward: ``teacher(recon)`` with ``recon`` not detached):

        | mode  | ``eval_input_grad`` | backward                                        | ``x.grad`` | parameters with gradients           |
        |-------|---------------------|-------------------------------------------------|------------|-------------------------------------|
        | train | any                 | ``train_full`` if full or x_rg, else ``heads``  | if x_rg    | path if full or x_rg, else heads    |
        | eval  | False               | ``heads``                                       | no, warns  | path if full (trunk: zeros), else heads |
        | eval  | True                | ``eval_full`` if full or x_rg, else ``heads``   | if x_rg    | path if full or x_rg, else heads    |

        heads = ``gate.*``, ``quality_heads.*`` (``lo_teacher_heads_backward_ex``: the reference as it executes); path = all
        but the semantic / style / prompt heads.  No graph at all when none of those parameters requires grad and ``x.grad`` is not due.
        ``train_full`` (kept forward + ``lo_teacher_full_backward_dx``; its scratch is 26 GB at batch 64, feature_dim 128): the reference's
        reentrant checkpoints see an input that requires grad and differentiate the whole trunk, whatever ``full_backward`` says.  The
        BatchNorm running statistics move once per forward (nothing is recomputed); the reference's reentrant recompute would advance
        them a second time.  ``eval_full`` (eval kept forward + ``lo_teacher_eval_backward``; the frozen reward model: deterministic,
        independent of the other samples of the batch): every BatchNorm differentiated at its running statistics, no dropout; running
        statistics, ``num_batches_tracked`` and the dropout stream (``drop_calls``) do not move.  If no parameter on the path requires
        grad (``teacher.requires_grad_(False)``) no parameter gradient is computed at all and ``x.grad`` has the same bits.  Its outputs
        come from the plain-form eval forward: they differ from the default (folded at feature_dim 128) eval forward at the fp16
        rounding level, like any two paths of ``lo_teacher_forward``.  The three other outputs stay non-differentiable."""
        self._ensure_flat()
        if torch.is_grad_enabled():
            route = teacher_route(self.training, self.eval_input_grad, self.all_parameters_live, x.requires_grad)
            if route.warn:
                warnings.warn("LunarMoETeacher in eval mode: the input requires grad but gets no gradient (its input gradient is built "
                              "for train mode only); outputs are the eval-mode forward's", UserWarning, stacklevel=2)
            live = [p for p in self._live_parameters(route.live_set) if p.requires_grad]
            if live or route.want_dx:
                q, w, st, pr, sem = _TeacherFunction.apply(self, route, x if route.want_dx else x.detach(), *live)
                return {"quality_scores": q, "expert_weights": w, "style_embedding": st, "prompt_embedding": pr,
                        "semantic_score": sem, "feature_maps": None}
        return self._native_forward(x)[0]
