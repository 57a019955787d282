"""The VAE half of ``TrainingManager._process_batch`` (reference: /root/reference/train_hybrid.py:838-954) as one
native sequence on the current HIP stream: forward + MSE/KL partial sums -> loss finalize -> backward ->
global-norm clip + AdamW -> (host) cosine-warm-restart LR.  No host synchronisation inside a step; metrics are
returned as a device tensor and only converted on request.

What is mirrored, line by line:
  :841-842  zero_grad            -> every gradient element is overwritten by the backward (no accumulation state)
  :850      vae(images)          -> lo_vae_forward (eps drawn on device unless injected)
  :859,862  recon_loss, kl_loss  -> fused partial sums + lo_vae_loss
  :886-889  vae_loss             -> (recon_weight - mean_advantage)*MSE + kl_weight*KL   (pg_loss = -mean(adv)*MSE)
  :895      / accumulation steps
  :907      optimizer steps only when (batch_idx+1) % accum == 0 — with the reference's zero_grad placement the
            gradients of the other micro-batches are discarded, so their backward is skipped here.  Opt-in,
            ``accumulate_gradients=True``: every micro-batch of a window takes its backward and the step sees their sum
            (lo_grad_accumulate) -- what the flag's name promises; off, nothing changes
  :913      clip_grad_norm_(max_grad_norm)   :921 AdamW(lr, wd=0.01, betas=(0.9,0.999))   :925 scheduler.step()
The teacher's contribution is the detached scalar ``mean_advantage``; it is an input here.
"""
from __future__ import annotations

import contextlib
import math
import os
from typing import Callable, Dict, Optional

import torch

from . import _lib
from .parallel import GradHandover, backward_phase, grad_range, set_linear_mode
from .vae import LunarisCoreVAE


def _alloc_scratch(nbytes: int, device: torch.device) -> torch.Tensor:
    """Device memory the steppers hand to kernels as pure scratch (the Gram scratch of the data-parallel norm; the teacher's scratch is
    its engine's): contents unspecified.  The poisoned-workspace tests swap this function; state the kernels accumulate into (the 1028-float
    optimizer scratch with its skipped-update counter, AdamW moments) is zero-initialised where it is created and is not scratch."""
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def cosine_warm_restarts_lr(base_lr: float, eta_min: float, t0: int, t_mult: int, epoch: int) -> float:
    """torch.optim.lr_scheduler.CosineAnnealingWarmRestarts after ``epoch`` calls of step() (train_hybrid.py:516-521)."""
    t_i, t_cur = t0, epoch
    while t_cur >= t_i:
        t_cur -= t_i
        t_i *= t_mult
    return eta_min + (base_lr - eta_min) * (1.0 + math.cos(math.pi * t_cur / t_i)) / 2.0


def decode_sprites_u8(u8_hwc: torch.Tensor) -> torch.Tensor:
    """uint8 [B,128,128,3] on the device -> normalised float32 [B,3,128,128] (train_hybrid.py:181-182), native kernel."""
    if u8_hwc.dtype != torch.uint8 or tuple(u8_hwc.shape[1:]) != (128, 128, 3) or not u8_hwc.is_cuda:
        raise ValueError("expected a CUDA uint8 tensor of shape [B,128,128,3]")
    u8_hwc = u8_hwc.contiguous()
    out = torch.empty(u8_hwc.shape[0], 3, 128, 128, dtype=torch.float32, device=u8_hwc.device)
    _lib.check(_lib.lib.lo_decode_sprites_u8(u8_hwc.data_ptr(), out.data_ptr(), u8_hwc.shape[0], _lib.stream_ptr()),
               "lo_decode_sprites_u8")
    return out


class LossScalePolicy:
    """GradScaler's policy (torch.cuda.amp.GradScaler, used by train_hybrid.py:917-923) for observations that LAG the device.

    `observe(scale, skipped_total, at, now)`: `skipped_total` = the device's count of skipped updates (non-finite gradient norm)
    after optimizer step `at`; `now` = the step the host has enqueued up to.  The host enqueues a step or two ahead of what it
    observes, so after one genuine overflow the steps already in the queue overflow too — at the OLD scale.  Those are the same
    overflow, not new ones (counting them cost 2-3 halvings and lost updates per event where GradScaler.update() costs
    one): of the updates skipped since the last observation, as many as ran before the last scale change are ignored; any beyond
    that ran at the current scale and halve it once.  `growth_interval` steps without a skip double it again, up to `init`."""

    def __init__(self, init: float = 65536.0, growth_interval: int = 2000):
        self.init, self.growth_interval = init, growth_interval
        self.skipped_seen, self.changed_at, self.last_obs = 0, 0, 0

    def observe(self, scale: float, skipped_total: int, at: int, now: int) -> float:
        new = skipped_total - self.skipped_seen
        at_old_scale = max(0, min(at, self.changed_at) - self.last_obs)      # steps of this window that ran before the change
        self.skipped_seen, self.last_obs = max(skipped_total, self.skipped_seen), max(at, self.last_obs)
        if new > at_old_scale:
            self.changed_at = now               # every step enqueued from now on runs at the new scale
            return max(1.0, scale * 0.5)
        if new <= 0 and scale < self.init and now - self.changed_at >= self.growth_interval:
            self.changed_at = now
            return min(self.init, scale * 2.0)
        return scale


class LossScaleObserver:
    """GradScaler's update (train_hybrid.py:917-923) without a host sync: the device's skipped-update counter is copied to pinned
    memory after optimizer steps (asynchronously) and evaluated when the copy has landed, i.e. one or two steps later.  Each
    observation carries the optimizer-step index it was taken after, so that updates skipped at a scale that has since been changed
    are not counted again (`LossScalePolicy`).  Data parallel (`fixed_lag`): the ranks must change the scale at the SAME step (the
    scale multiplies fp16 activation gradients, a rank at a higher scale can overflow alone), so there the observation taken `DP_LAG`
    steps earlier is waited for instead of polled -- a fixed lag, identical on every rank (the counters are: every rank sees the same
    averaged gradients).  `in_window`: an accumulation window is open.  Every micro-batch of a window runs at ONE loss scale (its
    factor blocks share one 1 / scale; the accumulator adds un-scaled gradients of one scale's fp16 range), so what is observed
    inside one is kept and the policy sees it when the window has ended or the next begins."""
    DP_LAG = 2      # data parallel: an observation is evaluated this many optimizer steps after it was enqueued

    def __init__(self, vae, policy: LossScalePolicy, counter: torch.Tensor):
        self.vae, self.policy, self.counter = vae, policy, counter
        self._slots = [torch.zeros(1, dtype=torch.float32).pin_memory() for _ in range(self.DP_LAG + 1)]
        self._inflight = []       # (event, pinned slot, optimizer-step index), oldest first
        self._deferred = []       # observations made inside a window: (skipped total, optimizer-step index)

    def window_begins(self, now: int) -> None:
        """The policy sees what was observed inside the previous window, so that the scale a window runs at is fixed before its
        first lo_vae_loss.  `now` = the optimizer step the host has enqueued up to."""
        pending, self._deferred = self._deferred, []
        for skipped_total, at in pending:
            self.vae.loss_scale = self.policy.observe(self.vae.loss_scale, skipped_total, at, now)

    def observed(self, skipped_total: float, at: int, now: int, in_window: bool = False) -> None:
        """One host-side observation of the device's skipped-update counter, taken after optimizer step `at`."""
        if in_window:
            self._deferred.append((int(skipped_total), at))
            return
        self.vae.loss_scale = self.policy.observe(self.vae.loss_scale, int(skipped_total), at, now)

    def step_enqueued(self, now: int, fixed_lag: bool) -> None:
        """Behind every optimizer step: the counter of the step just enqueued travels to pinned memory behind it; whichever earlier
        copy has landed by now is evaluated.  The host runs a step or two ahead of the GPU, so an overflow is answered after that
        many skipped updates — not after `--log_every` of them, as when only metrics() looked."""
        self.window_begins(now)           # accumulate_gradients: what metrics() saw inside the window that has just ended
        # (no window is open here: under accumulation the optimizer step is the last call of one, so `observed` applies at once)
        if fixed_lag:
            # wait for the observation of `DP_LAG` steps ago (long finished unless the host runs further ahead than that)
            while len(self._inflight) >= self.DP_LAG:
                ev, slot, at = self._inflight.pop(0)
                ev.synchronize()
                self.observed(float(slot[0]), at, now)
        else:
            while self._inflight and self._inflight[0][0].query():
                ev, slot, at = self._inflight.pop(0)
                self.observed(float(slot[0]), at, now)
        if len(self._inflight) < len(self._slots):
            busy = {id(s_) for _, s_, _ in self._inflight}
            slot = next(s_ for s_ in self._slots if id(s_) not in busy)
            slot.copy_(self.counter, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._inflight.append((ev, slot, now))


class AccumulationWindow:
    """Host bookkeeping of ``accumulate_gradients=True``: which of the k micro-batches of a window a call is.

    A window is the k consecutive calls that start at ``batch_idx % k == 0``; its last call, ``(batch_idx + 1) % k == 0``, is the one
    that steps (train_hybrid.py:907).  A call with ``batch_idx % k == 0`` always starts a new window and whatever an incomplete one
    had gathered is dropped (the end of an epoch whose length is no multiple of k).  A call that finds no window open starts one
    wherever it is (a run that begins in the middle of an epoch): that window is shorter than k and still ends at the reference's
    step.  ``advance`` returns (first, last, slot): slot = how many micro-batches of this window came before."""

    def __init__(self, k: int):
        self.k = max(1, int(k))
        self.count = 0          # micro-batches the open window holds; 0 = none open

    @property
    def open(self) -> bool:
        return self.count > 0

    def advance(self, batch_idx: int):
        first = batch_idx % self.k == 0 or self.count == 0
        slot = 0 if first else self.count
        if slot >= self.k:
            self.count = 0
            raise ValueError(f"accumulate_gradients: more than {self.k} calls without the end of a window (batch_idx {batch_idx}); "
                             "batch_idx must count the micro-batches of an epoch from 0")
        last = (batch_idx + 1) % self.k == 0
        self.count = 0 if last else slot + 1
        return first, last, slot

    def drop(self) -> None:
        self.count = 0


class VAEStepper:
    _swallows_keywords = False      # step(): an unknown keyword is an error (HybridStepper ignores them)

    def __init__(self, vae: LunarisCoreVAE, lr: float = 1e-4, min_lr: float = 1e-6, scheduler_t0: int = 10,
                 weight_decay: float = 0.01, max_grad_norm: float = 1.0, recon_weight: float = 1.0, kl_weight: float = 0.1,
                 gradient_accumulation_steps: int = 1, betas=(0.9, 0.999), eps: float = 1e-8,
                 grad_sync: Optional[Callable[[torch.Tensor], None]] = None, pipeline_optimizer: bool = False,
                 dp_factored_adamw: Optional[bool] = None, accumulate_gradients: bool = False,
                 ema_decay: float = 0.0, ema_every: int = 1, ema_warmup: bool = False):
        if not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1) (0 = no EMA), got {ema_decay}")
        if int(ema_every) < 1:
            raise ValueError(f"ema_every must be >= 1, got {ema_every}")
        _lib.require_gpu()
        self.vae = vae
        self.grad_sync = grad_sync      # data parallel: averages the flat gradient buffer across ranks (RCCL)
        if accumulate_gradients and self._dp_active():
            # accumulation under data parallel (one exchange of the accumulated buffers per window, k * world factor blocks) is not
            # built; an exchange object of one rank averages nothing and is not called in the mode
            raise NotImplementedError("accumulate_gradients=True is single process only (grad_sync with world > 1 is not built)")
        if getattr(vae, "attention", False) and self._dp_world() > 1:
            # the exchange ranges, the factor all-gather and the gathered-factor optimizer have never been run with the 86-tensor
            # layout: not offered untested
            raise NotImplementedError("data parallel (grad_sync with world > 1) is not built for LunarisCoreVAE(attention=True)")
        # pipeline_optimizer: the update of the Linear / decoder parameters (87 % of AdamW's 1.7 GB) and their operand refresh run
        # on the library's side stream beside the NEXT step's encoder forward (lo_vae_optimizer_step).  Parameters may then still
        # be in flight when step() returns: call synchronize_parameters() before touching them outside this stepper
        # (state_dict(), checkpoints, your own torch ops); forward / decode / sample through the module order themselves.
        self.pipeline_optimizer = bool(pipeline_optimizer)
        self._pipelined_engine = None
        self.base_lr, self.min_lr, self.t0 = lr, min_lr, scheduler_t0
        self.weight_decay, self.max_grad_norm = weight_decay, max_grad_norm
        self.recon_weight, self.kl_weight = recon_weight, kl_weight
        self.accum = max(1, int(gradient_accumulation_steps))
        self.betas, self.eps = betas, eps
        # The weight gradients of the three Linear layers (82 % of the parameters) are rank-B matrices: the fused step keeps them as
        # their factors -- norm from Gram matrices, gradient tiles formed inside the AdamW pass (csrc/lo_lowrank.hip) -- instead of
        # writing and re-reading 201 MB.  Single process, batch <= 128; LO_LINEAR_FACTORED=0: the materialised path (A/B).
        # `parameter_grads()` still returns all 72 gradients (the two matrices are written out on demand).
        knob = os.environ.get("LO_LINEAR_FACTORED", "1")
        self.linear_factored = grad_sync is None and knob != "0"
        # data parallel: the ranks all-gather the FACTORS (8.6 MB of fp16 per rank, exact) instead of exchanging the 201 MB of Linear
        # weight gradients, and each forms the averaged gradient from the gathered blocks (FlatGradSync.begin_factored)
        self.dp_factored = hasattr(grad_sync, "begin_factored") and knob != "0"
        # ... and, opt-in (LO_LINEAR_FACTORED=2, or dp_factored_adamw=True), never writes the averaged matrices either: norm and AdamW
        # read the gathered blocks (mode 3 of lo_vae_set_linear_factored; world * padded batch <= 512, else mode 2 as above)
        self.dp_factored_adamw = (knob == "2") if dp_factored_adamw is None else bool(dp_factored_adamw)
        self.dp_three_phase = True      # hand the encoder's last stage over before stages 3..1 run (False: one encoder range)
        # LO_EARLY_NORM=0 (A/B knob): no part of the norm is taken beside the encoder backward (the factored mode always takes its own)
        self._early_norm = os.environ.get("LO_EARLY_NORM", "1") != "0"
        flat = vae.flat_parameters()
        self.grads = torch.zeros_like(flat)
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.scratch = torch.zeros(1028, dtype=torch.float32, device=flat.device)   # [1024:1027] = norm, clip coef, finite
        self.losses = torch.zeros(4, dtype=torch.float32, device=flat.device)       # recon, kl, vae_loss, pg_loss
        self.opt_steps = 0
        self.last = None
        self._last_engine = None
        # the hand-over protocol of the data-parallel backward, and what the accumulation path shares with it (parallel.py)
        self._exchange = GradHandover(vae, self.grads, self.scratch, _alloc_scratch, early_norm=self._early_norm)
        # accumulate_gradients (opt-in; off: nothing below is touched): every micro-batch of a window takes its backward and the
        # window's last call steps on the sum -- `self.grads` is the accumulator, the first micro-batch's backward writes straight
        # into it, the others write `_stage` and lo_grad_accumulate adds them.  The two Linear matrices, while the factored mode
        # applies, are kept as one factor block per micro-batch (`GradHandover.factor_slots`) and never written out: the
        # gathered-factor passes of the data-parallel mode 3 read them, told to add instead of average (lo_vae_set_gathered_sum).
        self.accumulate = bool(accumulate_gradients)
        self._window = AccumulationWindow(self.accum) if self.accumulate else None
        self._win_batch = 0             # batch size of the open window
        self._stage: Optional[torch.Tensor] = None
        self._scale_policy = LossScalePolicy()
        self._loss_scale = LossScaleObserver(vae, self._scale_policy, self.scratch[1027:1028])
        # Weight EMA (opt-in; 0 = off: no buffer, no call, the step launches what it launches without the argument).  `ema` is an fp32
        # copy of the flat buffer that follows it by lo_vae_ema_update after every `ema_every`-th optimizer step (DESIGN.md section
        # 6d); evaluation, samples and checkpoints read it through ema_weights() / ema_state_dict().  Like the parameters it may
        # still be in flight after a pipelined step: synchronize_parameters() before reading it with your own torch ops.  Data
        # parallel needs no exchange: every rank applies the same update to the same parameters, so the averages are identical.
        self.ema_decay, self.ema_every, self.ema_warmup = float(ema_decay), int(ema_every), bool(ema_warmup)
        self.ema: Optional[torch.Tensor] = flat.clone() if self.ema_decay > 0 else None
        self.ema_steps = 0              # optimizer steps attempted since the average began (hostside.ema_decay_at's t)
        self.ema_updates = 0            # EMA passes enqueued (ema_steps // ema_every)
        self._ema_open = False          # inside ema_weights(): the flat buffer holds the average, the live weights are in a backup

    @property
    def lr(self) -> float:
        return cosine_warm_restarts_lr(self.base_lr, self.min_lr, self.t0, 2, self.opt_steps)

    def _dp_world(self) -> int:
        """Ranks of the exchange (`grad_sync.world`, which tests change between steps; 1 without an exchange object)."""
        return int(getattr(self.grad_sync, "world", 1))

    def _dp_linear_mode(self, eng, active: bool, early: bool) -> int:
        """`GradHandover.linear_mode` for this stepper's exchange object and flags as they are now."""
        return self._exchange.linear_mode(eng, self.grad_sync, self.dp_factored, self.dp_factored_adamw, active, early)

    def _dp_active(self) -> bool:
        """A data-parallel exchange is active: more than one rank, or an exchange object told to issue its collectives anyway."""
        return self._dp_world() > 1 or bool(getattr(self.grad_sync, "force", False))

    def step(self, images: torch.Tensor, batch_idx: int = 0, eps: Optional[torch.Tensor] = None,
             mean_advantage: float = 0.0, adv_dev: Optional[torch.Tensor] = None, **ignored):
        """One micro-batch.  Returns (recon, mu, logvar); losses stay on the device in ``self.losses``.  The one step body of both
        steppers: HybridStepper threads the teacher through `_objective_inputs`, `_drecon_seed` and `_behind_vae_work`.  Here an
        unknown keyword is a TypeError, as before; HybridStepper takes the advantage from its teacher and ignores `mean_advantage`,
        `adv_dev` and every other keyword it is given (its `step(images, batch_idx, eps, **_)` of before)."""
        if ignored and not self._swallows_keywords:
            raise TypeError(f"step() got an unexpected keyword argument {next(iter(ignored))!r}")
        vae = self.vae
        self._require_live_weights()
        images = images.detach().contiguous().float()
        # accumulate_gradients: every micro-batch of a window takes its gradients, the window's last call steps
        first, last, slot = self._window_advance(images.shape[0], batch_idx)
        takes_grads = last or self.accumulate
        recon, mu, logvar, eng = vae._native_forward(images, eps, target=images)
        st = _lib.stream_ptr()
        mean_advantage, adv_dev = self._objective_inputs(images, recon, takes_grads, mean_advantage, adv_dev, st)
        _lib.check(_lib.lib.lo_vae_loss(eng.handle, eng.ws.data_ptr(), self.recon_weight, self.kl_weight, float(mean_advantage),
                                        _lib.ptr(adv_dev), float(self.accum), self._chain_loss_scale(), self.losses.data_ptr(), st),
                   "lo_vae_loss")
        presummed = None
        if takes_grads:
            drecon = self._drecon_seed(eng, images, recon, first, st)
            presummed = self._backward(eng, images, recon, drecon, first, slot, last, st)
        if last:
            lr = self.lr
            self.opt_steps += 1
            self._clip_adamw(vae._flat, lr, st, eng, presummed)
            self._loss_scale.step_enqueued(self.opt_steps, fixed_lag=self._dp_world() > 1)
        if takes_grads:
            self._behind_vae_work(recon, first, last, st)
        self.last = (recon, mu, logvar)
        return recon, mu, logvar

    # ---- what HybridStepper overrides -----------------------------------------------------------------------------------------------
    def _objective_inputs(self, images, recon, takes_grads: bool, mean_advantage: float, adv_dev, st):
        """(mean_advantage, adv_dev) of lo_vae_loss; here the caller's."""
        return mean_advantage, adv_dev

    def _drecon_seed(self, eng, images, recon, first: bool, st) -> Optional[torch.Tensor]:
        """An explicit, un-scaled d vae_loss / d recon for the backward, or None: the final conv's backward forms the MSE gradient."""
        return None

    def _behind_vae_work(self, recon, first: bool, last: bool, st) -> None:
        """Behind the VAE's part of a call that takes gradients (on the last call of a window: behind its optimizer step)."""

    # ---- gradient accumulation (accumulate_gradients=True) ------------------------------------------------------------------------
    def _window_advance(self, batch: int, batch_idx: int):
        """(first, last, slot) of this call.  Off: every call is its own "window" and `last` is the reference's step rule.  On: the
        position in the window (`AccumulationWindow`); a new window first lets the loss-scale policy see what was observed inside the
        previous one, so that the scale it runs at is fixed before its first lo_vae_loss."""
        if not self.accumulate:
            return True, (batch_idx + 1) % self.accum == 0, 0
        first, last, slot = self._window.advance(batch_idx)
        if first:
            self._loss_scale.window_begins(self.opt_steps)
            self._win_batch = batch
        elif batch != self._win_batch:
            self._window.drop()
            raise ValueError(f"accumulate_gradients: every micro-batch of a window must have the same batch size (window of {self._win_batch}, "
                             f"got {batch} at batch_idx {batch_idx})")
        return first, last, slot

    def _window_open(self) -> bool:
        return self.accumulate and self._window.open

    def _window_factored(self, eng) -> bool:
        """The two Linear matrices of a window stay factor blocks: the factored mode is on, the batch is within its rank (128), the
        combined rank accum * padded batch is within what the gathered passes hold (512), and the model is the 72-tensor one (the
        gathered passes have never run with the attention layout).  Otherwise they are accumulated like every other gradient."""
        return (self.linear_factored and eng.batch <= 128 and not getattr(self.vae, "attention", False)
                and _lib.lib.lo_vae_gathered_scratch_bytes(eng.handle, self.accum) > 0)

    def _accumulate(self, acc: torch.Tensor, g: torch.Tensor, begin: int, end: int, st) -> None:
        """acc[begin:end] += g[begin:end] (lo_grad_accumulate; each micro-batch's gradients already carry 1 / accum)."""
        if end > begin:
            _lib.check(_lib.lib.lo_grad_accumulate(acc.data_ptr() + 4 * begin, g.data_ptr() + 4 * begin, end - begin, 1.0, 0, st),
                       "lo_grad_accumulate")

    def _chain_loss_scale(self) -> float:
        """The loss scale lo_vae_loss's seeds, the reward term and the backward are given.  Off: the model's.  On: times accum -- the
        seeds carry 1 / accum, and with the scale raised by as much the fp16 activation gradients of every micro-batch are the ones a
        plain step at accumulation 1 carries (no 1 / k taken out of fp16's range, the same roundings for a k that is no power of two);
        the backward's fp32 `1 / scale` applies the 1 / accum instead.  One value for a whole window (`LossScaleObserver`)."""
        return float(self.vae.loss_scale) * (self.accum if self.accumulate else 1)

    # ---- the backward: one interface, three paths -------------------------------------------------------------------------------------
    def _backward(self, eng, images: torch.Tensor, recon: torch.Tensor, drecon: Optional[torch.Tensor], first: bool, slot: int,
                  last: bool, st) -> Optional[int]:
        """Native backward of the fused loss into ``self.grads`` (micro-batches 2..k of an accumulation window: into the staging
        buffer, then added).  drecon: the un-scaled d vae_loss / d recon as an explicit seed (``fused = 2``: the latent seeds stay
        lo_vae_loss's) instead of the MSE gradient the final conv's backward forms itself -- the hybrid step's reward-gradient
        objective.  Returns the presummed begin for the optimizer step: the flat index from which on the gradients' share of the norm
        already lies in scratch[512..1024), or None when that step has to take the whole norm."""
        self._last_engine = eng
        if not first and self._stage is None:
            self._stage = torch.zeros_like(self.grads)
        G = self.grads if first else self._stage
        bargs = (images.data_ptr(), self.vae._flat.data_ptr(), eng.ws.data_ptr(), recon.data_ptr(), images.data_ptr(),
                 1 if drecon is None else 2, _lib.ptr(drecon), None, None, self._chain_loss_scale(), G.data_ptr(), st)
        # `accumulate` is fixed at construction; `grad_sync` is not (bench.py sets it to None for its rank-local leg)
        if self.accumulate:
            return self._backward_accumulating(eng, bargs, G, first, slot, last)
        if hasattr(self.grad_sync, "begin"):
            return self._exchange.backward(eng, bargs, self.grad_sync, self._dp_active(), self.dp_factored, self.dp_factored_adamw,
                                           self.dp_three_phase)
        return self._backward_single(eng, bargs)

    def _backward_accumulating(self, eng, bargs, G: torch.Tensor, first: bool, slot: int, last: bool) -> Optional[int]:
        """One micro-batch's backward into the window's accumulator `self.grads`: the first writes it (every element: nothing of an
        earlier window survives), the others write the staging buffer and are added.  Factored: the phased backward (data-parallel
        mode 3) leaves this micro-batch's factor block, which is copied to its slot; the two matrices are in neither buffer.  No
        backward of a window takes any part of the gradient norm (no scratch set): the norm is that of the sum, taken at the end --
        behind the window's last backward, factored, the norm's share of everything from fc_mu.weight on (the accumulated flat buffer,
        and the Gram matrices of the filled factor blocks for the two matrices, cross terms between micro-batches included) goes to
        scratch[512..1024) and the blocks are left to the optimizer step; materialised, that step takes the whole norm."""
        st = bargs[-1]
        _lib.check(_lib.lib.lo_vae_set_gradnorm_scratch(eng.handle, None), "lo_vae_set_gradnorm_scratch")
        n = self.grads.numel()
        factored = self._window_factored(eng)
        if factored:
            set_linear_mode(eng, 3)
            _lib.check(_lib.lib.lo_vae_set_gathered_sum(eng.handle, 1), "lo_vae_set_gathered_sum")
            _lib.check(_lib.lib.lo_vae_set_async_handover(eng.handle, 0), "lo_vae_set_async_handover")
            backward_phase(eng, 1, bargs)
            backward_phase(eng, 2, bargs)
            fo, fb = grad_range(eng, "lo_vae_factor_block")
            slots = self._exchange.factor_slots(eng, self.accum, fb)
            slots[slot * fb:(slot + 1) * fb].copy_(eng.ws[fo:fo + fb])
            h_end, d_beg, d_end = self._exchange.linear_matrix_bounds(eng)
            ranges = ((0, grad_range(eng, "lo_vae_linear_grad_range")[0]), (h_end, d_beg), (d_end, n))
        else:
            set_linear_mode(eng, 0)
            _lib.check(_lib.lib.lo_vae_backward(eng.handle, *bargs), "lo_vae_backward")
            ranges = ((0, n),)
        if not first:
            for b, e in ranges:
                self._accumulate(self.grads, G, b, e, st)
        if not (last and factored):
            return None
        self._exchange.norm_of_gathered(eng, slots[:(slot + 1) * fb], slot + 1)
        return grad_range(eng, "lo_vae_phase1_grad_range")[0]

    def _backward_single(self, eng, bargs) -> Optional[int]:
        """Single process (or a plain `grad_sync` callable): the backward takes the sum of squares of everything from fc_mu.weight on
        as soon as it is final, beside the encoder backward; _clip_adamw then reads only the encoder range for the norm."""
        fac = self.linear_factored and eng.batch <= 128
        set_linear_mode(eng, 1 if fac else 0)
        early = self.grad_sync is None and (fac or self._early_norm)
        _lib.check(_lib.lib.lo_vae_set_gradnorm_scratch(eng.handle, self.scratch.data_ptr() if early else None),
                   "lo_vae_set_gradnorm_scratch")
        _lib.check(_lib.lib.lo_vae_backward(eng.handle, *bargs), "lo_vae_backward")
        if self.grad_sync is not None:
            self.grad_sync(self.grads)
        elif _lib.lib.lo_vae_gradnorm_presummed(eng.handle):
            return grad_range(eng, "lo_vae_phase1_grad_range")[0]
        return None

    def synchronize_parameters(self) -> None:
        """Make the current stream wait for a pipelined optimizer step's side-stream work (no-op otherwise)."""
        if self._pipelined_engine is not None:
            _lib.check(_lib.lib.lo_vae_join(self._pipelined_engine.handle, _lib.stream_ptr()), "lo_vae_join")

    def _clip_adamw(self, flat: torch.Tensor, lr: float, st, eng, presummed: Optional[int]) -> None:
        """clip_grad_norm_ + AdamW on the VAE's flat buffers (train_hybrid.py:913,921), through the engine in both orders (LO_OPT_SERIAL =
        norm, AdamW, re-pack in order on this stream): its clip kernel reads the plan's rendezvous-failure word and skips the update on
        the device when a fused-GroupNorm wait of this step ran out.  presummed: what the step's backward returned (`_backward`)."""
        flags = (1 if presummed is not None else 0) | (0 if self.pipeline_optimizer else 2)
        _lib.check(_lib.lib.lo_vae_optimizer_step(eng.handle, flat.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(),
                                                  self.exp_avg_sq.data_ptr(), eng.ws.data_ptr(), float(self.max_grad_norm), float(lr),
                                                  float(self.betas[0]), float(self.betas[1]), float(self.eps), float(self.weight_decay),
                                                  self.opt_steps, self.scratch.data_ptr(), flags, st), "lo_vae_optimizer_step")
        self.vae.mark_weights_changed()
        eng.packed_version = self.vae._current_version()     # this engine's operand copies were refreshed by the call itself
        if self.pipeline_optimizer:
            self._pipelined_engine = eng
        self._ema_after_step(flat, st, eng)

    # ---- weight EMA (ema_decay > 0) --------------------------------------------------------------------------------------------------
    @property
    def ema_decay_now(self) -> float:
        """The per-step decay the next optimizer step's EMA runs at (`hostside.ema_decay_at`: `ema_decay`, lower during warm-up)."""
        from .hostside import ema_decay_at
        return ema_decay_at(self.ema_decay, self.ema_steps, self.ema_warmup)

    def _ema_after_step(self, flat: torch.Tensor, st, eng) -> None:
        """Right behind an optimizer step: every `ema_every`-th one moves the average, with the per-step decay of THIS step
        (`ema_decay_now`) raised to the power `ema_every` -- the weight the average would have kept over the steps it sat out.  The
        pass is gated by the step's norm block, so an update the device skipped leaves the average's bits alone; through the engine
        it is ordered behind the pipelined AdamW on the library's side stream (lo_vae_ema_update)."""
        if self.ema is None:
            return
        from .hostside import ema_one_minus_decay
        decay = self.ema_decay_now
        self.ema_steps += 1
        if self.ema_steps % self.ema_every != 0:
            return
        omd = ema_one_minus_decay(decay, self.ema_every)
        _lib.check(_lib.lib.lo_vae_ema_update(eng.handle, flat.data_ptr(), self.ema.data_ptr(), omd, self.scratch.data_ptr(), st),
                   "lo_vae_ema_update")
        self.ema_updates += 1

    def _require_ema(self) -> None:
        if self.ema is None:
            raise RuntimeError("this stepper keeps no weight EMA (construct it with ema_decay > 0)")

    def _require_live_weights(self) -> None:
        if self._ema_open:
            raise RuntimeError("step() inside ema_weights(): the model holds the averaged weights; leave the block before training on")

    def _join_engines(self) -> None:
        """The current stream waits for the side-stream work of EVERY engine of the model (operand refreshes read the flat buffer)."""
        for eng in self.vae._engines.values():
            _lib.check(_lib.lib.lo_vae_join(eng.handle, _lib.stream_ptr()), "lo_vae_join")

    def ema_state_dict(self):
        """The averaged weights under the model's ``state_dict`` keys (CPU clones, cut from the EMA buffer at the parameters' flat
        offsets): ``LunarisCoreVAE.load_state_dict`` and the reference's ``LunarCoreVAE.load_state_dict`` take it."""
        from collections import OrderedDict
        from .hostside import flat_offsets
        self._require_ema()
        self.synchronize_parameters()
        vp = OrderedDict(self.vae.named_parameters())
        offs = flat_offsets(vp, self.vae.flat_parameters())
        keys = list(self.vae.state_dict().keys())
        assert keys == list(vp.keys()), "the VAE's state_dict holds its parameters and nothing else"
        return OrderedDict((k, self.ema[offs[k]:offs[k] + vp[k].numel()].detach().cpu().reshape(vp[k].shape).clone()) for k in keys)

    @contextlib.contextmanager
    def ema_weights(self):
        """``with stepper.ema_weights():`` -- inside the block the model computes with the averaged weights (``vae(x)``, ``decode``,
        ``sample``, ``Validator``, every engine of every batch size); on exit the live weights are back bit for bit.  A content
        swap through one backup buffer: flat -> backup, EMA -> flat on entry, backup -> flat on exit, each followed by
        ``mark_weights_changed()`` so that every engine re-packs its operands from what the flat buffer then holds (a pack is a
        function of the fp32 values alone, so the operands of the live weights come back bit for bit as well).  The backup (the
        size of the flat buffer) lives only while the block is open.  ``step()`` inside the block raises; blocks do not nest."""
        self._require_ema()
        if self._ema_open:
            raise RuntimeError("ema_weights() blocks do not nest")
        vae = self.vae
        flat = vae.flat_parameters()
        self.synchronize_parameters()          # the pipelined AdamW and the EMA pass behind it
        self._join_engines()                   # ... and whatever else still reads the flat buffer on a side stream
        backup = flat.clone()
        flat.copy_(self.ema)
        vae.mark_weights_changed()
        self._ema_open = True
        try:
            yield vae
        finally:
            self._join_engines()               # operand refreshes of the averaged weights may still be reading the flat buffer
            flat.copy_(backup)
            vae.mark_weights_changed()
            self._ema_open = False

    def decode_sprites(self, u8_hwc: torch.Tensor) -> torch.Tensor:
        """uint8 [B,128,128,3] on the device -> normalised float32 [B,3,128,128] (`decode_sprites_u8`)."""
        return decode_sprites_u8(u8_hwc)

    def metrics(self) -> Dict[str, float]:
        """Host copy of the last step's scalars (this synchronises the stream)."""
        v = torch.cat([self.losses, self.scratch[1024:1028], self._sync_fail_word()]).cpu().tolist()
        self._check_sync(v[8])
        self._loss_scale.observed(v[7], self.opt_steps, self.opt_steps, self._window_open())
        return {"recon_loss": v[0], "kl_loss": v[1], "vae_loss": v[2], "pg_loss": v[3], "grad_norm": v[4],
                "clip_coef": v[5], "grads_finite": v[6], "lr": self.lr, "skipped_steps": v[7], "loss_scale": self.vae.loss_scale}

    def _sync_fail_word(self) -> torch.Tensor:
        """The engines' "a fused-GroupNorm rendezvous ran out" words (lo_vae_sync_fail_word), summed, as one float."""
        words = [e.sync_fail for e in self.vae._engines.values()]
        if not words:
            return torch.zeros(1, dtype=torch.float32, device=self.losses.device)
        return torch.stack([w.float().sum() for w in words]).sum().reshape(1)

    @staticmethod
    def _check_sync(word: float) -> None:
        if word != 0:
            raise _lib.LunarisHipError("a fused GroupNorm epilogue gave up waiting for the other workgroups of its sample (a launch of a "
                                       "step did not complete).  No parameter update has been applied since: the optimizer's clip kernel "
                                       "reads the same word and skips the update on the device.  LO_GNB_APPLY_FUSE=0 / LO_GN_FUSE=0 run "
                                       "the separate passes")

    def check_device_health(self) -> None:
        """Host-synchronising look at the rendezvous-failure word (checkpoints call it before they write anything)."""
        self._check_sync(float(self._sync_fail_word().item()))

    def flat_grads(self) -> torch.Tensor:
        """The flat gradient buffer with every gradient of the last step in it (in the factored mode the two Linear weight
        gradients are written out first; `self.grads` alone does not hold them then)."""
        self.parameter_grads()
        return self.grads

    def parameter_grads(self):
        """Views of the flat gradient buffer, one per parameter (state_dict order).  In the factored mode the two Linear weight
        gradients of the last step are written out first (`lo_vae_materialize_linear_grads`: the tiles the AdamW pass formed).
        With ``accumulate_gradients`` these are the gradients accumulated over the last COMPLETE window (the matrices from its factor
        blocks); inside a window the buffers are half-filled and asking for them is an error."""
        if self._window_open():
            raise RuntimeError("accumulate_gradients: the gradients are complete after the last call of a window, not inside one")
        for eng in self.vae._engines.values():
            if eng is self._last_engine and _lib.lib.lo_vae_linear_factored(eng.handle):
                _lib.check(_lib.lib.lo_vae_materialize_linear_grads(eng.handle, eng.ws.data_ptr(), self.grads.data_ptr(), _lib.stream_ptr()),
                           "lo_vae_materialize_linear_grads")
        return [self.grads[o:o + n].view(shape) for (o, n, shape) in self.vae._layout]


class HybridStepper(VAEStepper):
    """Full `_process_batch` (train_hybrid.py:838-954): VAE step + the teacher, as the reference EXECUTES it.

    Per micro-batch: VAE forward; teacher(images) (its result is dead in the reference — the prompt embedding it
    produces is overwritten before use, lunar_evaluator.py:438 — but it runs in train mode, so its BatchNorm
    running-statistics update is a real side effect and is kept; `run_dead_teacher_call=False` skips it); losses;
    teacher(recon.detach()); reward / EMA baseline / advantage on the device (`lo_hybrid_reward`); the VAE objective
    with the detached mean advantage; VAE backward + clip + AdamW; teacher_loss backward for the only parameters that
    receive gradients in the reference (gate, quality_heads: SURVEY §3.2) + clip + AdamW on exactly those.
    Teacher dropout (the module's ``dropout_rate``, 0.1 like the reference unless constructed otherwise) is applied in both
    teacher calls, each with its own call seed; the heads' backward replays the masks of the evaluated call."""

    _swallows_keywords = True       # step(images, batch_idx, eps, **_): the objective's inputs are the teacher's, whatever is passed

    def __init__(self, vae: LunarisCoreVAE, teacher, teacher_lr: float = 1e-4, quality_weight: float = 0.5, reward_scale: float = 0.1,
                 semantic_weight: float = 0.5, baseline_momentum: float = 0.9, run_dead_teacher_call: bool = True,
                 teacher_full_backward: bool = False, reward_grad_weight: float = 0.0, **kw):
        super().__init__(vae, **kw)
        self.teacher = teacher
        # opt-in: the VAE also climbs the frozen (eval-mode) teacher's quality score, vae_loss -= weight * mean(q_eval) / accum with
        # q_eval = quality_scores of the teacher in eval mode on recon, NOT detached; the teacher's parameters are constants in the term
        # (DESIGN.md "Reward gradient").  0: the step makes exactly the calls it makes without the argument
        self.reward_grad_weight = float(reward_grad_weight)
        if self.reward_grad_weight < 0:
            raise ValueError("reward_grad_weight must be >= 0")
        self._rg = None                 # per-batch buffers of the reward pass (_reward_grad_seed)
        # the teacher trained "as documented" -- every parameter on the path of the teacher loss gets its gradient
        # (lo_teacher_full_backward: the reference with non-reentrant checkpoints) and its AdamW update; off = the reference as it
        # executes (gate + quality heads only)
        self.teacher_full_backward = bool(teacher_full_backward)
        self.teacher_base_lr = teacher_lr
        self.quality_weight, self.reward_scale = quality_weight, reward_scale
        self.semantic_weight, self.baseline_momentum = semantic_weight, baseline_momentum
        self.run_dead_teacher_call = run_dead_teacher_call
        dev = vae.flat_parameters().device
        self.reward_state = torch.zeros(2, dtype=torch.float32, device=dev)     # baseline, initialised flag
        self.reward_out = torch.zeros(8, dtype=torch.float32, device=dev)
        self.adv_dev = torch.zeros(1, dtype=torch.float32, device=dev)
        self.reward_grad_out = torch.zeros(2, dtype=torch.float32, device=dev)   # reward term of vae_loss, mean(q_eval)
        self.seed_coef = torch.zeros(1, dtype=torch.float32, device=dev)         # un-scaled MSE coefficient of d vae_loss / d recon
        self._t_stage = None                     # accumulate_gradients: the teacher gradients of micro-batches 2..k before they are added
        self._t_ready = False                    # t_range, t_grads, t_m, t_v, t_scratch exist (_teacher_setup)
        self._t_checkpoint = None                # a checkpoint's teacher optimizer state until then (load_teacher_optimizer_state)
        self.last_teacher_out = None             # outputs of the last train-mode teacher(recon)

    @property
    def teacher_optimizer_ready(self) -> bool:
        """The teacher's optimizer state (`t_range`, `t_grads`, `t_m`, `t_v`, `t_scratch`) exists: a step has run."""
        return self._t_ready

    def load_teacher_optimizer_state(self, state: dict) -> None:
        """The teacher optimizer state of a checkpoint (hostside.restore_checkpoint): applied to `t_m` / `t_v` now if they exist,
        else when the first step makes them."""
        self._t_checkpoint = state
        if self._t_ready:
            self._apply_teacher_checkpoint()

    def _apply_teacher_checkpoint(self) -> None:
        from collections import OrderedDict
        from .hostside import flat_offsets, load_adamw_state_dict
        state, self._t_checkpoint = self._t_checkpoint, None
        t, (b, e) = self.teacher, self.t_range
        tp = OrderedDict(t.named_parameters())
        offs = flat_offsets(tp, t._flat)
        rel = {k: (o - b if b <= o < e else 0) for k, o in offs.items()}
        names = list(tp.keys())
        live = {"state": {i: st for i, st in state.get("state", {}).items() if b <= offs[names[int(i)]] < e}}
        load_adamw_state_dict(live, tp, self.t_m, self.t_v, rel)

    def _teacher_setup(self, batch: int) -> None:
        """What the stepper owns of the teacher's update, made at the first step: the flat gradient, AdamW moments over `t_range`, the
        optimizer scratch.  Everything per batch size (workspaces, rows, ranges) is the teacher engine's."""
        if self._t_ready:
            return
        t = self.teacher
        b, e = self.t_range = (0, t._flat.numel()) if self.teacher_full_backward else t._engine(batch).heads_range
        self.t_grads = torch.zeros_like(t._flat)
        self.t_m = torch.zeros(e - b, dtype=torch.float32, device=t._flat.device)
        self.t_v = torch.zeros(e - b, dtype=torch.float32, device=t._flat.device)
        self.t_scratch = torch.zeros(1028, dtype=torch.float32, device=t._flat.device)
        self._t_ready = True
        if self._t_checkpoint is not None:
            self._apply_teacher_checkpoint()

    # ---- the hooks of VAEStepper.step -------------------------------------------------------------------------------------------------
    def _objective_inputs(self, images, recon, takes_grads: bool, mean_advantage, adv_dev, st):
        """Between the VAE forward and lo_vae_loss: the teacher calls and the reward.  The advantage is the device's (`adv_dev`)."""
        t, B = self.teacher, images.shape[0]
        if self.run_dead_teacher_call:
            t.update_statistics_only(images)            # train_hybrid.py:853-855 (side effects only)
        # train_hybrid.py:865 (no autograd node: the head gradients are taken below).  Full-backward mode: the plain forward that keeps
        # every block's output for lo_teacher_full_backward (only on the micro-batches whose gradients are used)
        tout = t._native_forward(recon, mode="keep" if self.teacher_full_backward and takes_grads else "auto")[0]
        self.last_teacher_out = tout
        self._teacher_setup(B)
        q_rows, s_rows, n_rows = tout["quality_scores"], tout["semantic_score"], B
        if self._dp_active():
            # data parallel: the baseline / advantage are functions of the batch means only (train_hybrid.py:870-883);
            # one 5-float all-reduce keeps them identical on every rank
            means = torch.cat([q_rows.mean(dim=0), s_rows.mean(dim=0)]).contiguous()
            self.grad_sync.average_small(means)
            self._reward_rows = (means[:4].reshape(1, 4).contiguous(), means[4:5].reshape(1, 1).contiguous())
            q_rows, s_rows = self._reward_rows
            n_rows = 1
        _lib.check(_lib.lib.lo_hybrid_reward(q_rows.data_ptr(), s_rows.data_ptr(), n_rows,
                                             float(self.semantic_weight), float(self.reward_scale), float(self.baseline_momentum),
                                             float(self.quality_weight), float(self.accum), self.reward_state.data_ptr(),
                                             self.reward_out.data_ptr(), self.adv_dev.data_ptr(), st), "lo_hybrid_reward")
        return 0.0, self.adv_dev

    # `_teacher_grads` reads what the train-mode teacher(recon) of this call left (the kept tensors in bws, the pooled features and
    # logits in ws, the call's dropout stream).  One rule places it: with a reward pass (`reward_grad_weight > 0`) it runs BEFORE that
    # pass, whose eval forward overwrites all of this (`_drecon_seed`); otherwise at the end of the call's VAE work
    # (`_behind_vae_work`).  The teacher's update stays last either way.
    def _drecon_seed(self, eng, images, recon, first: bool, st) -> Optional[torch.Tensor]:
        if self.reward_grad_weight <= 0:
            return None
        self._teacher_grads(self.teacher, recon, self.last_teacher_out, first)
        return self._reward_grad_seed(self.teacher, eng, images, recon, st)

    def _behind_vae_work(self, recon, first: bool, last: bool, st) -> None:
        if self.reward_grad_weight <= 0:
            self._teacher_grads(self.teacher, recon, self.last_teacher_out, first)
        if last:
            # the VAE's optimizer step of this call has counted itself already: the teacher's schedule is at the step before
            t_lr = cosine_warm_restarts_lr(self.teacher_base_lr, self.min_lr, self.t0, 2, self.opt_steps - 1)
            self._teacher_update(self.teacher, recon, t_lr, st)

    def _teacher_grads(self, t, recon, tout, first: bool = True) -> None:
        """teacher_loss.backward() into ``self.t_grads`` (train_hybrid.py:891-904): the gate and the quality heads
        (`heads_backward`), or with ``teacher_full_backward`` every parameter on the loss path (`full_backward` on the evaluated images,
        under non-reentrant checkpoints).  Reads what the train-mode teacher(recon) of this step left.  first = False
        (``accumulate_gradients``, micro-batches 2..k of a window): into the staging buffer, then added to ``t_grads`` over `t_range`
        (both backwards write every element of it)."""
        coef = float(self.quality_weight) / float(self.accum)
        if not first and self._t_stage is None:
            self._t_stage = torch.zeros_like(self.t_grads)
        out = self.t_grads if first else self._t_stage
        if self.teacher_full_backward:
            # accumulate_gradients: the fp16 activation gradients stay where a plain step's are (coef carries 1 / accum, gscale gives
            # it back; the fp32 parameter gradients come out un-scaled either way) -- at gscale alone the smallest of them, in the
            # feature extractor, lose bits to fp16's subnormal range: 1e-4 on its first conv's gradient at accum = 2
            from .teacher import loss_gscale
            gscale = loss_gscale(recon.shape[0]) * self.accum if self.accumulate else None
            t.full_backward(recon, tout["expert_weights"], coef, gscale=gscale, out=out)
        else:
            t.heads_backward(tout["expert_weights"], coef, out=out)
        if not first:
            self._accumulate(self.t_grads, out, *self.t_range, _lib.stream_ptr())

    def _reward_grad_seed(self, t, eng, images, recon, st) -> torch.Tensor:
        """The reward pass of a ``reward_grad_weight`` step, after lo_vae_loss: the teacher in EVAL mode on recon (running statistics,
        no dropout; `_native_forward(mode="keep_eval")` moves no byte of its state and not its dropout stream), the term's scalars
        (lo_vae_reward_term), and its backward with no parameter gradients (`_native_backward` with a seed), whose last kernel stores the
        complete d vae_loss / d recon = d(-w mean(q_eval) / accum) / d recon + c (recon - images) into the persistent seed buffer returned.
        The fp16 activation gradients run at the operating point the eval-gradient tests pin (upstream rows of -2, gscale 2**20);
        the objective's coefficient w / (8 B accum) multiplies the fp32 result."""
        B = recon.shape[0]
        if self._rg is None or self._rg["B"] != B:
            f32 = dict(dtype=torch.float32, device=recon.device)
            emb = torch.zeros(2, B, t.embedding_dim, **f32)
            self._rg = {"B": B, "q": torch.zeros(B, 4, **f32), "w": torch.zeros(B, t.num_experts, **f32), "emb": emb,
                        "sem": torch.zeros(B, 1, **f32), "up": torch.full((B, 4), -2.0, **f32), "seed": torch.zeros(B, 3, 128, 128, **f32)}
            self._rg["out"] = (self._rg["q"], self._rg["w"], emb[0], emb[1], self._rg["sem"])
        rg = self._rg
        teng = t._native_forward(recon, mode="keep_eval", out=rg["out"])[1]
        _lib.check(_lib.lib.lo_vae_reward_term(eng.handle, eng.ws.data_ptr(), rg["q"].data_ptr(), self.reward_grad_weight, float(self.accum),
                                               self._chain_loss_scale(), self.losses.data_ptr(), self.reward_grad_out.data_ptr(),
                                               self.seed_coef.data_ptr(), st), "lo_vae_reward_term")
        t._native_backward(teng, "eval_full", recon, teng.saved_views(), rg["w"], rg["up"], None, (0.0, 0), None, rg["seed"],
                           seed=(images, self.seed_coef, self.reward_grad_weight / (8.0 * B * float(self.accum))))
        return rg["seed"]

    def _teacher_update(self, t, recon, t_lr: float, st) -> None:
        """clip + AdamW on the gradients of `_teacher_grads` over `t_range` (train_hybrid.py:914, 922).  The reference as it executes:
        the gate and the quality heads only (train_hybrid.py:891-904), one flat range, which the head kernels read in fp32 -- no
        re-pack needed.  ``teacher_full_backward``: every teacher parameter live (lo_teacher_clip_adamw_full); the conv / attention
        operands are packed fp16 copies and are re-packed before the next forward."""
        b, e = self.t_range
        eng = t._engine(recon.shape[0]) if self.teacher_full_backward else None
        if self.grad_sync is not None:
            self.grad_sync(self.t_grads[b:e])
        args = (float(self.max_grad_norm), float(t_lr), float(self.betas[0]), float(self.betas[1]), float(self.eps),
                float(self.weight_decay), self.opt_steps, self.t_scratch.data_ptr(), st)
        if self.teacher_full_backward:
            _lib.check(_lib.lib.lo_teacher_clip_adamw_full(eng.handle, t._flat.data_ptr(), self.t_grads.data_ptr(), self.t_m.data_ptr(),
                                                           self.t_v.data_ptr(), *args), "lo_teacher_clip_adamw_full")
            t.mark_weights_changed()
        else:
            _lib.check(_lib.lib.lo_clip_adamw_step(t._flat[b:e].data_ptr(), self.t_grads[b:e].data_ptr(), self.t_m.data_ptr(),
                                                   self.t_v.data_ptr(), e - b, *args), "lo_clip_adamw_step(teacher)")

    def metrics(self) -> Dict[str, float]:
        """The 12 scalars of train_hybrid.py:929-942 (+ grad norm / lr); one host copy."""
        v = torch.cat([self.losses, self.scratch[1024:1027], self.reward_out[:7], self.scratch[1027:1028], self._sync_fail_word(),
                       self.reward_grad_out]).cpu().tolist()
        self._check_sync(v[15])
        recon, kl, vae_loss, pg = v[0:4]
        q_loss, sem_r, q_r, baseline, adv, t_loss, q_mean = v[7:14]
        self._loss_scale.observed(v[14], self.opt_steps, self.opt_steps, self._window_open())
        return {"recon_loss": recon, "kl_loss": kl, "quality_loss": q_loss, "pg_loss": pg, "semantic_reward": sem_r,
                "quality_reward": q_r, "baseline": baseline, "advantage": adv, "vae_loss": vae_loss, "teacher_loss": t_loss,
                "total_loss": vae_loss + t_loss, "quality_scores": q_mean, "grad_norm": v[4], "clip_coef": v[5],
                "grads_finite": v[6], "lr": self.lr, "skipped_steps": v[14], "loss_scale": self.vae.loss_scale,
                "reward_grad_loss": v[16], "eval_quality": v[17]}
