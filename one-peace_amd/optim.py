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

``ShardedFusedAdamW`` / ``ShardedTorchAdamW`` are the reference's ``use_distributed_fused_adam: true`` (optim/adam.py:58-70 -> apex's
DistributedFusedAdam): the moments, the master and the average are kept for this rank's ranges of ``distributed.shard_layout`` alone, the
same kernel runs over them, and the parameters are gathered after the step.  Every rank's slice is bit for bit the unsharded step's.

Deviation from the reference, stated, for the memory-efficient arrangement only: global-norm clipping multiplies the gradient by
the clip coefficient in fp32 inside the update kernel; the reference scales its bf16 gradients in place first
(fairseq/utils.py:393-397: one extra bf16 rounding).  With master weights the reference itself multiplies fp32 gradients
(fp16_optimizer.py: _sync_fp16_grads_to_fp32, clip_grad_norm, _unscale_grads), so there the kernel's order is the reference's."""
import re

import torch

from . import hip, ops
from .distributed import FlatParameters, gather_shards, resolve_shard, shard_layout


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


def _checked_ema(ema, flat, layout=None):
    """layout: the ``distributed.ShardLayout`` of a sharded optimiser (None: the optimiser keeps the whole state, and so must the EMA)."""
    if ema is not None and ema.flat is not flat:
        raise ValueError("the FlatEMA was built over other FlatParameters than this optimiser")
    if ema is not None and getattr(ema, "layout", None) != layout:
        raise ValueError("the FlatEMA keeps %s, this optimiser %s: a sharded optimiser needs FlatEMA(shard=(rank, world)) with its own "
                         "rank and world, an unsharded one the full average" % (_layout_name(ema.layout), _layout_name(layout)))
    return ema


def _layout_name(layout):
    return "the whole buffer" if layout is None else "the shard of rank %d of %d" % (layout.rank, layout.world)


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


def _torch_scaled_grad(flat, grad_scale, clip_norm, has_master):
    """(g, norm) of the torch statement: the fp32 gradient of the WHOLE flat buffer times grad_scale and the clip coefficient, and the
    unclipped norm (None without clipping).  The norm is global, so a sharded step forms it over the full buffer as well."""
    g = flat.grads.float() * grad_scale
    norm = g.norm() if clip_norm > 0 else None
    if norm is not None and has_master:
        # a flat fp32 norm over millions of elements is off by up to ~4e-4 relative on the CPU; the bf16 rounding of the other
        # arrangement hides that, an fp32 master does not (the reference sums per-parameter norms): accumulate in fp64
        norm = torch.linalg.vector_norm(g, dtype=torch.float64).float()
    if norm is not None:
        g = g * (clip_norm / (norm + 1e-6)).clamp(max=1.0)  # fairseq/utils.py:349-397
    return g, norm


def _torch_adamw_range(opt, g, start, end, local):
    """The rule of ``TorchAdamW`` on the elements [start, end) of the flat buffers, stated once for it and ``ShardedTorchAdamW``.
    g: the scaled and clipped fp32 gradient of the whole buffer; ``opt.exp_avg``, ``opt.exp_avg_sq`` and ``opt.master`` hold the range
    from index ``local`` on (0 and the whole buffer for ``TorchAdamW``).  Every operation is elementwise: a range gives its elements
    what the whole buffer gives them."""
    f, (b1, b2), n = opt.flat, opt.betas, end - start
    g = g[start:end]
    exp_avg, exp_avg_sq = opt.exp_avg[local:local + n], opt.exp_avg_sq[local:local + n]
    exp_avg.mul_(b1).add_(g, alpha=1 - b1)
    exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
    update = exp_avg / (exp_avg_sq.sqrt() + opt.eps)
    bias = (1 - b2 ** opt.step_count) ** 0.5 / (1 - b1 ** opt.step_count)
    for g_start, g_end, scale, decays in f.groups:
        a, b = max(g_start, start), min(g_end, end)
        if b <= a:
            continue
        mast = None if opt.master is None else opt.master[a - start + local:b - start + local]
        pf = f.params[a:b].float() if mast is None else mast
        if decays and opt.weight_decay != 0:
            pf = pf + pf * (-opt.weight_decay * opt.lr * scale)
        new = pf - opt.lr * scale * bias * update[a - start:b - start]
        if mast is not None:
            mast.copy_(new)
            new = mast.to(f.params.dtype)
        f.params[a:b].copy_(new)


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
        f = self.flat
        g, norm = _torch_scaled_grad(f, grad_scale, clip_norm, self.master is not None)
        _torch_adamw_range(self, g, 0, f.numel, 0)
        if self.ema is not None:
            self.ema.step()
        if f.params.is_cuda:
            ops.refresh_weight_cache()
        return norm

    def zero_grad(self):
        self.flat.zero_grad()


class _ShardedState:
    """What ``ShardedFusedAdamW`` and ``ShardedTorchAdamW`` share: the layout, the ``[shard | tail]`` state buffers and the gather."""

    def _init_state(self, flat, lr, betas, eps, weight_decay, rank, world, process_group, master_weights, ema):
        self.flat, self.pg = flat, process_group
        rank, world = resolve_shard(rank, world, process_group)
        self.layout = shard_layout(flat.numel, world, rank)
        self.rank, self.world = rank, world
        self.ema = _checked_ema(ema, flat, self.layout)
        self.lr, self.betas, self.eps, self.weight_decay = lr, betas, eps, weight_decay
        self.exp_avg = torch.zeros(self.layout.local_numel, dtype=torch.float32, device=flat.params.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.master = self.layout.take(flat.params.detach()).float() if master_weights else None
        self.step_count = 0

    def set_lr(self, lr):
        self.lr = lr

    @torch.no_grad()
    def sync_master(self):
        """Re-read this rank's two ranges of the fp32 master from ``flat.params`` (after an outside write)."""
        if self.master is None:
            raise RuntimeError("sync_master: this optimiser was built without master_weights")
        for a, b, lo in self.layout.ranges:
            self.master[lo:lo + b - a].copy_(self.flat.params[a:b])

    def gather_params(self):
        """Every rank's updated shard into every rank's ``flat.params``: one ``all_gather_into_tensor`` over
        ``flat.params[:world * S8 * 8]`` (``distributed.gather_shards``: in place over RCCL).  The tail was updated by every rank."""
        gather_shards(self.flat.params, self.layout, self.pg)

    def state_bytes(self):
        """Bytes of optimiser state this rank holds: both moments, the master and the EMA average if kept, 4 B per element each."""
        return 4 * self.layout.local_numel * (2 + (self.master is not None) + (self.ema is not None))

    def step(self, grad_scale=1.0, clip_norm=0.0):
        """``step_local`` (no collective), ``gather_params``, then the refresh of the derived weight copies.  Returns the gradient
        norm as ``FusedAdamW.step`` does.  The gradients must have been all-reduced (``BucketedGradReducer``): every rank holds the
        full reduced gradient, the clip norm is taken over the full buffer and is the same bits on every rank."""
        norm = self.step_local(grad_scale, clip_norm)
        self.gather_params()
        if self.flat.params.is_cuda:
            ops.refresh_weight_cache()
        return norm

    def zero_grad(self):
        self.flat.zero_grad()


class ShardedFusedAdamW(_ShardedState):
    """``FusedAdamW`` with the optimiser state partitioned over the data-parallel ranks: the reference's
    ``use_distributed_fused_adam: true`` (optim/adam.py:58-70 -> apex's DistributedFusedAdam), which all three shipped
    configurations set.  ``distributed.shard_layout`` says what a rank owns: ``exp_avg``, ``exp_avg_sq`` and the optional ``master`` are
    fp32 tensors of ``8 * (S8 + tail8)`` elements, laid out ``[shard | tail]``; the tail (fewer than ``world`` vectors) is replicated.
    With all four streams the state is 16 B/param / world instead of 16 B/param per GPU.

    Every rank's slice comes out bit for bit as ``FusedAdamW`` stores it: the same kernel runs over the range with the global group
    table (``hip.adamw_step_shard``), the clip norm is ``hip.sqnorm`` of the full reduced gradient buffer as in the unsharded step, and
    the rule does not depend on where an element lies.  Gradients are all-reduced as before; a reduce-scatter is not part of this.

    rank, world: default to the process group's; explicit values without an initialised group make one process stand in for a rank
    (``step_local`` then works, the collective ``step`` does not).  ``ema``: an ``ema.FlatEMA(flat, shard=(rank, world))`` of the same
    rank and world; it is updated inside the shard and tail launches.  Same ``set_lr`` / ``zero_grad`` / ``sync_master`` as ``FusedAdamW``.
    Out of scope: capturing the sharded step in a ``TrainStepGraph`` or a CUDA graph (the collective between the launches and the
    weight-cache refresh has not been captured or tested)."""

    def __init__(self, flat: FlatParameters, lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05, rank=None, world=None,
                 process_group=None, master_weights=False, ema=None):
        if not flat.params.is_cuda or flat.params.dtype != torch.bfloat16:
            raise RuntimeError("ShardedFusedAdamW needs bf16 parameters on an MI355X (the HIP path has no CPU fallback)")
        self._init_state(flat, lr, betas, eps, weight_decay, rank, world, process_group, master_weights, ema)
        groups = [g for g in flat.groups if g[1] > g[0]]
        dev = flat.params.device
        self._end8 = torch.tensor([g[1] // 8 for g in groups], dtype=torch.int64, device=dev)  # the GLOBAL table, as FusedAdamW's
        self._scale = torch.tensor([g[2] for g in groups], dtype=torch.float32, device=dev)
        self._wd = torch.tensor([weight_decay if g[3] else 0.0 for g in groups], dtype=torch.float32, device=dev)
        assert groups and groups[0][0] == 0 and groups[-1][1] == flat.numel and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))

    def step_local(self, grad_scale=1.0, clip_norm=0.0):
        """The shard launch and a second launch of the same entry over the tail.  No collective; parameters outside the two ranges
        are not touched."""
        self.step_count += 1
        f = self.flat
        sq = hip.sqnorm(f.grads) if clip_norm > 0 else None
        keep, take = self.ema.coefficients(self.ema.num_updates + 1) if self.ema is not None else (0.0, 0.0)
        for a, b, lo in self.layout.ranges:
            own = slice(lo, lo + b - a)
            hip.adamw_step_shard(f.params, f.grads, a // 8, (b - a) // 8, self.exp_avg[own], self.exp_avg_sq[own],
                                 None if self.master is None else self.master[own], None if self.ema is None else self.ema.shadow[own],
                                 self._end8, self._scale, self._wd, self.lr, self.betas[0], self.betas[1], self.eps, self.step_count,
                                 keep, take, grad_scale, sq, clip_norm)
        if self.ema is not None:
            self.ema.num_updates += 1
        return sq.sqrt() * abs(grad_scale) if sq is not None else None


class ShardedTorchAdamW(_ShardedState):
    """``ShardedFusedAdamW`` stated with torch ops: ``TorchAdamW``'s rule (``_torch_adamw_range``) on this rank's two ranges, any device
    or dtype.  The CPU control-flow runs over gloo use it, and it is the readable statement of what a rank computes."""

    def __init__(self, flat: FlatParameters, lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05, rank=None, world=None,
                 process_group=None, master_weights=False, ema=None):
        self._init_state(flat, lr, betas, eps, weight_decay, rank, world, process_group, master_weights, ema)

    @torch.no_grad()
    def step_local(self, grad_scale=1.0, clip_norm=0.0):
        self.step_count += 1
        g, norm = _torch_scaled_grad(self.flat, grad_scale, clip_norm, self.master is not None)
        for a, b, lo in self.layout.ranges:
            _torch_adamw_range(self, g, a, b, lo)
        if self.ema is not None:
            self.ema.step()
        return norm
