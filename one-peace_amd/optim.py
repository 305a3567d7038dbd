"""Fused AdamW over flat bf16 parameters.

Update rule = the reference's in-repo ``Adam`` (one_peace/optim/adam.py:186-253; what runs when apex is absent): fp32 moments, fp32
math, decoupled weight decay applied before the Adam update, eps added to sqrt(v).  Param groups = the reference's
(trainer.py:265-278 -> utils/layer_decay.py:34-77): no weight decay for ``ndim <= 1`` / ``.bias`` / ``no_weight_decay()`` names,
and -- with ``layer_decay < 1`` -- the lr of layer id i scaled by ``layer_decay ** (L + 1 - i)`` (optim/base_optimizer.py:8-14).
ONE HIP launch over the flat buffers of ``distributed.FlatParameters`` per step, whatever the number of groups (a device table
maps ranges to their lr scale / weight decay).

Two arrangements of the bf16 parameters, as the reference has them (trainer.py:297-307):

  * ``master_weights=False`` (default) -- ``MemoryEfficientFP16Optimizer`` (``memory_efficient_bf16: true``): the parameters exist in
    bf16 only; the step widens them to fp32, updates and rounds straight back.  22 bytes/parameter of HBM traffic.  An update
    smaller than half a bf16 spacing (2^-9 |p|) is rounded away, every step, and never accumulates.
  * ``master_weights=True`` -- ``FP16Optimizer`` (``bf16: true`` alone; optim/fp16_optimizer.py:13-250): a flat fp32 master copy is
    what Adam updates, and the bf16 parameters are its cast after every step.  28 bytes/parameter of traffic and +4 bytes/parameter
    of memory: +15.6 GB at the 4B model, against 267 of 309 GB reserved at the headline batch.

Both optimisers take ``ema=``, an ``ema.FlatEMA`` over the same flat buffers: the reference trainer's fp32 weight average
(trainer.py:243-250, :895-907), updated from the new bf16 parameters inside the same launch (+8 bytes/parameter).

Deviation from the reference, stated, for the memory-efficient arrangement only: global-norm clipping multiplies the gradient by
the clip coefficient in fp32 inside the update kernel; the reference scales its bf16 gradients in place first
(fairseq/utils.py:393-397: one extra bf16 rounding).  With master weights the reference itself multiplies fp32 gradients
(fp16_optimizer.py: _sync_fp16_grads_to_fp32, clip_grad_norm, _unscale_grads), so there the kernel's order is the reference's."""
import re

import torch

from . import hip, ops
from .distributed import FlatParameters


def layer_id_of(var_name, num_max_layer):
    """one_peace/utils/layer_decay.py:8-21 (get_num_layer): adapters' embeddings -> 0, adapter rel_pos_table k and encoder
    layer k -> k + 1, everything else (projections, logit scale, final norms) -> the last id."""
    for ad in ("text_adapter", "image_adapter", "audio_adapter"):
        if var_name.startswith(ad):
            rest = var_name[len(ad) + 1:]
            return int(rest.split(".")[1]) + 1 if rest.startswith("rel_pos_table") else 0
    if var_name.startswith("fusion_model.layers"):
        return int(var_name.split(".")[2]) + 1
    return num_max_layer - 1


def reference_param_groups(model, num_layers=None, layer_decay=1.0):
    """(no_decay(name, p), lr_scale(name, p)) callables for ``FlatParameters`` that reproduce trainer.py:265-278."""
    skip = set(model.no_weight_decay()) if hasattr(model, "no_weight_decay") else set()

    def no_decay(name, p):
        name = re.sub("^module.module.", "", name)
        return p.ndim <= 1 or name.endswith(".bias") or name in skip

    if num_layers is None or layer_decay >= 1.0:
        return no_decay, None
    values = [layer_decay ** (num_layers + 1 - i) for i in range(num_layers + 2)]

    def lr_scale(name, p):
        name = re.sub("^module.module.", "", name)
        return values[layer_id_of(re.sub("^encoder_wrapper.", "", name), len(values))]
    return no_decay, lr_scale


def _checked_ema(ema, flat):
    if ema is not None and ema.flat is not flat:
        raise ValueError("the FlatEMA was built over other FlatParameters than this optimiser")
    return ema


class FusedAdamW:
    """master_weights=True keeps ``self.master``, an fp32 copy of ``flat.params`` taken at construction: the step updates the master
    and writes ``flat.params`` as its bf16 cast, without reading it.  Anything written into ``flat.params`` from outside afterwards
    (weights loaded into the model once the optimiser exists) must be followed by ``sync_master()``: otherwise the next step
    overwrites it with the cast of the old master.
    ema: an ``ema.FlatEMA`` over the same ``flat``.  The step then updates the fp32 weight average from the new bf16 parameters in the
    same launch (with or without the master) and advances ``ema.num_updates``; nothing else has to call ``ema.step()``."""

    def __init__(self, flat: FlatParameters, lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05, master_weights=False, ema=None):
        if not flat.params.is_cuda or flat.params.dtype != torch.bfloat16:
            raise RuntimeError("FusedAdamW needs bf16 parameters on an MI355X (the HIP path has no CPU fallback)")
        self.flat = flat
        self.master = flat.params.float() if master_weights else None
        self.ema = _checked_ema(ema, flat)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros(flat.numel, dtype=torch.float32, device=flat.params.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.step_count = 0
        groups = [g for g in flat.groups if g[1] > g[0]]
        dev = flat.params.device
        self._end8 = torch.tensor([g[1] // 8 for g in groups], dtype=torch.int64, device=dev)
        self._scale = torch.tensor([g[2] for g in groups], dtype=torch.float32, device=dev)
        self._wd = torch.tensor([weight_decay if g[3] else 0.0 for g in groups], dtype=torch.float32, device=dev)
        assert groups and groups[0][0] == 0 and groups[-1][1] == flat.numel and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))

    def set_lr(self, lr):
        """optim/base_optimizer.py:8-14: the scheduled lr; group g runs at lr * lr_scale_g."""
        self.lr = lr

    def sync_master(self):
        """Re-read the fp32 master from ``flat.params`` (fp16_optimizer.py: build_fp32_params, after an outside write)."""
        if self.master is None:
            raise RuntimeError("sync_master: this optimiser was built without master_weights")
        self.master.copy_(self.flat.params)

    def step(self, grad_scale=1.0, clip_norm=0.0):
        """grad_scale multiplies the gradient inside the kernel (1/world_size after a SUM all-reduce, trainer.py:917-923).
        clip_norm > 0: the reference's global-norm clipping (trainer.py:929 -> fairseq/utils.py:349-397) -- the norm is
        one extra pass over the flat gradient buffer, the clip coefficient is derived on the device inside the update
        kernel.  Returns the (unclipped, scaled) gradient norm as a device scalar when clipping is on.
        A non-finite gradient norm makes the whole step non-finite: with a NaN anywhere in the gradients every parameter and both
        moments come out NaN (``TorchAdamW`` does the same), nothing is stepped quietly with the unclipped gradient.  The returned
        norm is what a training loop should check before it steps, as the reference does (trainer.py:830-837 raises
        FloatingPointError); without clipping no norm is computed and a NaN gradient reaches its own element only."""
        self.step_count += 1
        f = self.flat
        sq = hip.sqnorm(f.grads) if clip_norm > 0 else None
        if self.ema is not None:  # the average of the new bf16 parameters, in the same launch (ema.py)
            keep, take = self.ema.coefficients(self.ema.num_updates + 1)
            hip.adamw_step_groups_ema(f.params, self.master, f.grads, self.exp_avg, self.exp_avg_sq, self.ema.shadow, self._end8,
                                      self._scale, self._wd, self.lr, self.betas[0], self.betas[1], self.eps, self.step_count, keep,
                                      take, grad_scale, sq, clip_norm)
            self.ema.num_updates += 1
        elif self.master is None:
            hip.adamw_step_groups(f.params, f.grads, self.exp_avg, self.exp_avg_sq, self._end8, self._scale, self._wd, self.lr,
                                  self.betas[0], self.betas[1], self.eps, self.step_count, grad_scale, sq, clip_norm)
        else:
            hip.adamw_step_groups_master(f.params, self.master, f.grads, self.exp_avg, self.exp_avg_sq, self._end8, self._scale,
                                         self._wd, self.lr, self.betas[0], self.betas[1], self.eps, self.step_count, grad_scale, sq,
                                         clip_norm)
        ops.refresh_weight_cache()  # the raw-pointer update does not bump _version: refresh the dgrad copies in one launch
        return sq.sqrt() * abs(grad_scale) if sq is not None else None

    def zero_grad(self):
        self.flat.zero_grad()


class TorchAdamW:
    """The same update over ``FlatParameters`` written with torch ops (fp32 math on the flat buffers, any device / dtype): the
    optimiser of the CPU control-flow runs of the data-parallel step (``bench.py --debug-cpu-micro``, world-size-4 gloo test) and
    a readable statement of what the fused kernel computes.  Same interface as ``FusedAdamW``, ``master_weights`` included: with
    it the fp32 ``self.master`` is what the rule reads and writes, and ``flat.params`` receives its cast.  With ``ema`` the step ends
    with ``ema.step()``."""

    def __init__(self, flat: FlatParameters, lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05, master_weights=False, ema=None):
        self.flat = flat
        self.master = flat.params.float() if master_weights else None
        self.ema = _checked_ema(ema, flat)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros(flat.numel, dtype=torch.float32, device=flat.params.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.step_count = 0

    def set_lr(self, lr):
        self.lr = lr

    def sync_master(self):
        if self.master is None:
            raise RuntimeError("sync_master: this optimiser was built without master_weights")
        self.master.copy_(self.flat.params)

    @torch.no_grad()
    def step(self, grad_scale=1.0, clip_norm=0.0):
        self.step_count += 1
        f, (b1, b2) = self.flat, self.betas
        g = f.grads.float() * grad_scale
        norm = g.norm() if clip_norm > 0 else None
        if norm is not None and self.master is not None:
            # a flat fp32 norm over millions of elements is off by up to ~4e-4 relative on the CPU; the bf16 rounding of the other
            # arrangement hides that, an fp32 master does not (the reference sums per-parameter norms): accumulate in fp64
            norm = torch.linalg.vector_norm(g, dtype=torch.float64).float()
        if norm is not None:
            g = g * (clip_norm / (norm + 1e-6)).clamp(max=1.0)  # fairseq/utils.py:349-397
        self.exp_avg.mul_(b1).add_(g, alpha=1 - b1)
        self.exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
        update = self.exp_avg / (self.exp_avg_sq.sqrt() + self.eps)
        bias = (1 - b2 ** self.step_count) ** 0.5 / (1 - b1 ** self.step_count)
        for start, end, scale, decays in f.groups:
            if end <= start:
                continue
            pf = f.params[start:end].float() if self.master is None else self.master[start:end]
            if decays and self.weight_decay != 0:
                pf = pf + pf * (-self.weight_decay * self.lr * scale)
            new = pf - self.lr * scale * bias * update[start:end]
            if self.master is not None:
                self.master[start:end].copy_(new)
                new = self.master[start:end].to(f.params.dtype)
            f.params[start:end].copy_(new)
        if self.ema is not None:
            self.ema.step()
        if f.params.is_cuda:
            ops.refresh_weight_cache()
        return norm

    def zero_grad(self):
        self.flat.zero_grad()
