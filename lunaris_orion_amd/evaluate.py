"""Held-out validation: what the model does on sprites the optimizer never saw.

The reference builds a ``val_loader`` over a tenth of the dataset (train_hybrid.py:552-573) and names the early-stopping argument
``validation_loss`` (:216), then feeds it the mean of the logged training losses (:1049) and never reads the loader.  ``Validator``
is the pass the names promise: per held-out sprite the reconstruction MSE, the KL term, PSNR and SSIM, and with a teacher its
eval-mode quality score, summed ON THE DEVICE (lo_eval.hip) so that a whole pass ends in one device-to-host copy.

The forward is ``lo_vae_forward`` with an explicit all-zero ``eps``: z = mu, so the result is a function of the weights and the
sprite alone (no noise to average over, the KL term does not depend on it anyway) and two passes over the same weights agree bit
for bit.  What a pass leaves untouched: the noise stream (``_seed``, ``noise_calls``, ``next_eps`` -- the entry point is called
directly, not through ``_native_forward``), every optimizer buffer, the loss scale, the teacher's BatchNorm statistics and counters,
its dropout stream and its ``training`` flag (the scores come from ``_native_forward(mode="keep_eval")``, the forward of the
reward-gradient objective), the reward baseline, and torch's generators.  What it does touch is the engine's one workspace: the
generation counters are bumped, so a backward of an earlier forward of that batch size fails as after any other forward.
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional

import torch

from . import _lib
from .trainer import decode_sprites_u8
from .vae import LunarisCoreVAE

#: slots of the device accumulator (lo_eval_accumulate, include/lunaris_hip.h)
ACC_COUNT, ACC_MSE, ACC_KL, ACC_PSNR, ACC_SSIM, ACC_QUALITY, ACC_PSNR_MIN, ACC_PSNR_MAX = range(8)


class Validator:
    """``Validator(stepper_or_vae, teacher=None, weights="live").run(batches, n_valid_per_batch) -> dict``.

    Given a stepper (``VAEStepper`` / ``HybridStepper``) the pass uses its model, loss weights, gradient exchange (data parallel) and,
    unless ``teacher`` is passed, its teacher; given a bare ``LunarisCoreVAE`` the reference's default weights (1.0, 0.1).

    A validator computes at ONE batch size, that of the first batch it is handed -- in the CLI the training step's, so
    the pass runs on the step's engine and workspace and no second one is created for the odd-sized tail of the split
    (``data.val_batches`` pads that tail by repeating a sprite and says how many rows count, ``n_valid``).  A batch with fewer rows is
    filled up the same way here, one with more is taken in chunks.  The reason is more than memory: the launch plan of the forward
    depends on the batch size (tiles, K splits), so the last bits of a sample's losses do too; at one batch size a metric does not
    depend on how the caller cut the held-out set into batches, nor on what the padding rows hold."""

    def __init__(self, stepper_or_vae, teacher=None, weights: str = "live"):
        _lib.require_gpu()
        if weights not in ("live", "ema"):
            raise ValueError(f"weights must be 'live' or 'ema', got {weights!r}")
        if isinstance(stepper_or_vae, LunarisCoreVAE):
            self.stepper, self.vae = None, stepper_or_vae
        else:
            self.stepper, self.vae = stepper_or_vae, stepper_or_vae.vae
        self.teacher = teacher if teacher is not None else getattr(self.stepper, "teacher", None)
        self.recon_weight = float(getattr(self.stepper, "recon_weight", 1.0))
        self.kl_weight = float(getattr(self.stepper, "kl_weight", 0.1))
        self.grad_sync = getattr(self.stepper, "grad_sync", None)
        # "ema": every pass runs inside stepper.ema_weights() -- the averaged weights, the live ones back bit for bit afterwards -- and
        # says so in its result ("val_weights": "ema"); "live" is the pass as it has always been
        self.weights = weights
        if weights == "ema" and getattr(self.stepper, "ema", None) is None:
            raise ValueError("weights='ema' needs a stepper that keeps a weight EMA (VAEStepper(..., ema_decay > 0))")
        self.batch: Optional[int] = None               # pinned by the first batch
        self._bufs: Dict[int, dict] = {}
        self._acc: Optional[torch.Tensor] = None

    def _buffers(self, B: int, device: torch.device) -> dict:
        buf = self._bufs.get(B)
        if buf is None:
            f32 = dict(dtype=torch.float32, device=device)
            L = self.vae.latent_dim
            buf = {"recon": torch.empty(B, 3, 128, 128, **f32), "mu": torch.empty(B, L, **f32), "logvar": torch.empty(B, L, **f32),
                   "eps": torch.zeros(B, L, **f32), "img": torch.empty(B, 2, **f32), "kl": torch.empty(B, **f32), "teacher": None}
            t = self.teacher
            if t is not None:
                buf["teacher"] = tuple(torch.empty(B, n, **f32) for n in (4, t.num_experts, t.embedding_dim, t.embedding_dim, 1))
            self._bufs[B] = buf
        return buf

    def forward(self, images: torch.Tensor) -> dict:
        """The deterministic forward of one batch (z = mu) into this validator's buffers: ``lo_vae_forward`` on the engine of that
        batch size with eps = 0, and the eval-mode teacher on the reconstruction.  Returns the buffers (recon, mu, logvar, ...)."""
        vae = self.vae
        if images.dim() != 4 or tuple(images.shape[1:]) != (3, 128, 128) or not images.is_cuda:
            raise ValueError(f"expected a CUDA tensor of shape [B, 3, 128, 128], got {tuple(images.shape)}")
        images = images.detach().contiguous().float()
        B = images.shape[0]
        if self.stepper is not None:
            self.stepper.synchronize_parameters()      # a pipelined optimizer step may still be writing the parameters
        eng = vae._engine(B)
        buf = self._buffers(B, images.device)
        eng.gen_enc += 1                               # the workspace's activations are this forward's from here on
        eng.gen_dec += 1
        _lib.check(_lib.lib.lo_vae_forward(eng.handle, images.data_ptr(), buf["eps"].data_ptr(), 0, vae._flat.data_ptr(), eng.ws.data_ptr(),
                                           buf["recon"].data_ptr(), buf["mu"].data_ptr(), buf["logvar"].data_ptr(), None,
                                           _lib.stream_ptr()), "lo_vae_forward")
        if self.teacher is not None:
            self.teacher._native_forward(buf["recon"], mode="keep_eval", out=buf["teacher"])
        return buf

    def _add_batch(self, batch: torch.Tensor, n_valid: int) -> None:
        """Adds the first `n_valid` rows of one batch to the pass, at THIS validator's batch size (see the class docstring): more rows
        are taken in chunks of it, a short chunk is filled up by repeating its first row, a chunk of padding alone is not run."""
        images = decode_sprites_u8(batch) if batch.dtype == torch.uint8 else batch.detach().contiguous().float()
        rows = images.shape[0]
        if not 0 <= n_valid <= rows:
            raise ValueError(f"n_valid {n_valid} outside [0, {rows}]")
        if self.batch is None:
            self.batch = rows
        B, st = self.batch, _lib.stream_ptr()
        for start in range(0, n_valid, B):
            chunk, valid = images[start:start + B], min(n_valid - start, B)
            if chunk.shape[0] < B:
                chunk = torch.cat([chunk, chunk[:1].expand(B - chunk.shape[0], -1, -1, -1)])
            chunk = chunk.contiguous()
            buf = self.forward(chunk)
            _lib.check(_lib.lib.lo_eval_image_metrics(buf["recon"].data_ptr(), chunk.data_ptr(), B, valid, buf["img"].data_ptr(), st),
                       "lo_eval_image_metrics")
            _lib.check(_lib.lib.lo_eval_latent_kl(buf["mu"].data_ptr(), buf["logvar"].data_ptr(), B, self.vae.latent_dim, valid,
                                                  buf["kl"].data_ptr(), st), "lo_eval_latent_kl")
            quality = buf["teacher"][0] if buf["teacher"] is not None else None
            _lib.check(_lib.lib.lo_eval_accumulate(buf["img"].data_ptr(), buf["kl"].data_ptr(), _lib.ptr(quality), valid,
                                                   self._acc.data_ptr(), st), "lo_eval_accumulate")

    def run(self, batches: Iterable[torch.Tensor], n_valid_per_batch: Iterable[int]) -> Dict[str, float]:
        """One pass.  batches: device tensors, uint8 [B,128,128,3] (as the feeder delivers them) or float [B,3,128,128] in [-1, 1];
        n_valid_per_batch: how many leading rows of each count.  Keys: val_recon_loss, val_kl_loss, val_loss (= recon_weight * recon +
        kl_weight * kl: no policy-gradient term), val_psnr, val_psnr_min, val_psnr_max, val_ssim, val_quality (with a teacher) and
        n.  Per-sample means over the held-out sprites of ALL ranks; n = 0 gives NaN for every metric.  ``weights="ema"``: the same
        pass on the stepper's averaged weights, plus ``"val_weights": "ema"``."""
        if self.weights == "ema":
            with self.stepper.ema_weights():
                out = self._run(batches, n_valid_per_batch)
            out["val_weights"] = "ema"
            return out
        return self._run(batches, n_valid_per_batch)

    def _run(self, batches: Iterable[torch.Tensor], n_valid_per_batch: Iterable[int]) -> Dict[str, float]:
        dev = self.vae.flat_parameters().device
        if self._acc is None or self._acc.device != dev:
            self._acc = torch.zeros(8, dtype=torch.float64, device=dev)
        self._acc.zero_()
        for batch, n_valid in zip(batches, n_valid_per_batch):
            self._add_batch(batch, int(n_valid))
        acc = self._acc
        sync = self.grad_sync
        if sync is not None and (getattr(sync, "world", 1) > 1 or getattr(sync, "force", False)):
            # every rank validated its stride: the sums and the count through the small-tensor exchange (mean of the sums x world),
            # the extremes as maxima; every rank then finalises the same numbers and takes the same decisions
            sums = acc[:ACC_PSNR_MIN].clone()
            sync.average_small(sums)
            sums *= float(sync.world)
            none = torch.full((2,), -math.inf, dtype=torch.float64, device=dev)
            ext = torch.where(acc[ACC_COUNT] > 0, torch.stack([-acc[ACC_PSNR_MIN], acc[ACC_PSNR_MAX]]), none)
            sync.max_small(ext)
            acc = torch.cat([sums, torch.stack([-ext[0], ext[1]])])
        v = acc.cpu().tolist()                         # the pass's one device-to-host copy
        n = int(round(v[ACC_COUNT]))
        mean = (lambda s: s / n) if n > 0 else (lambda s: float("nan"))
        recon, kl = mean(v[ACC_MSE]), mean(v[ACC_KL])
        out = {"val_recon_loss": recon, "val_kl_loss": kl, "val_loss": self.recon_weight * recon + self.kl_weight * kl,
               "val_psnr": mean(v[ACC_PSNR]), "val_psnr_min": v[ACC_PSNR_MIN] if n > 0 else float("nan"),
               "val_psnr_max": v[ACC_PSNR_MAX] if n > 0 else float("nan"), "val_ssim": mean(v[ACC_SSIM])}
        if self.teacher is not None:
            out["val_quality"] = mean(v[ACC_QUALITY])
        out["n"] = n
        return out
