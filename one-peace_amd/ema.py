"""Exponential moving average of the weights, in fp32, over the flat buffers of ``distributed.FlatParameters``.

What the reference trainer keeps beside its optimiser (one_peace/trainer.py): built at :243-250 (``cfg.ema.store_ema`` ->
``EMAModule``), stepped after every update at :895-907 (``ema.step(model, num_updates)``, ``ema_decay`` logged), saved at :394-399
(``extra_state["ema"]`` and ``["ema_fp32_params"]``) and restored at :574-595.  Here the average is ONE fp32 tensor as long as
``flat.params`` (``shadow``), updated by one HIP launch -- on its own (``hip.ema_step``, 10 B/param) or inside the AdamW launch
(``optim.FusedAdamW(ema=...)``, 8 B/param on top of the step) -- instead of a cast, a ``mul_`` and an ``add_`` per parameter.

The rule, stated once and used by every route:

    keep = float32(decay_at(updates))      take = float32(1.0 - decay_at(updates))      (the subtraction in double, as Python does it)
    e'   = fmaf(take, p, fl32(keep * e))   p: the bf16 parameter as stored after the optimiser step, e: the fp32 average
    decay_at(updates) = 0 if updates < start_update else decay                           (utils/ema_module.py:154-158)

which is bit for bit what torch computes on a CPU for the two lines of fairseq/fairseq/modules/ema_module.py:101-127,
``ema.mul_(decay); ema.add_(param.to(ema.dtype), alpha=1 - decay)``.  With decay 0 it gives e' = p exactly.  The average always
follows the bf16 parameter, also beside an optimiser with ``master_weights=True``: the reference's EMA reads the model, never the
optimiser's fp32 copy.

Two facts about the reference (checked with torch 2.10 on a CPU; tests/golden/ema.pt holds the evidence of the first):

  1. one_peace/utils/ema_module.py as the trainer calls it does NOT average.  Its loop walks ``new_model.state_dict().items()``
     (:115); those tensors are detached, so ``not param.requires_grad`` (:139) is true for every key and every parameter takes the
     copy branch: after a step with decay 0.999 its "EMA" is bit-identical to the new weights.  The vendored fairseq class walks
     ``named_parameters()`` and does average; the unmodified one_peace class does too when ``state_dict()`` keeps ``requires_grad``
     (``keep_vars=True``).  The averaging rule is what is built here.
  2. An EMA stored in bf16 (``ema_fp32: false``) does nothing at the default decay: with decay 0.9999, 50 steps towards weights 1.5
     times larger changed 0 of 2^18 elements, because ``take * p`` is below half a bf16 spacing of e.  So only the fp32 average
     exists here and ``ema_fp32=False`` is refused.

Shard mode (``FlatEMA(flat, shard=(rank, world))``, beside ``optim.ShardedFusedAdamW``): the rank keeps the average of its ranges of
``distributed.shard_layout`` only, ``[shard | tail]``, 4 B/param / world.  The rule is elementwise, so every element of the average
is bit for bit the full average's; what needs the whole average (``full_shadow``, ``fp32_params``, ``ema_state``, ``applied``,
``reverse``) is then COLLECTIVE: every rank must call it.

Out of scope: ``ema_update_freq`` (the one_peace trainer never reads it) and ``ema_seed_model``."""
import contextlib
import struct
from collections import OrderedDict

import torch

from . import hip, ops
from .distributed import FlatParameters, gather_full, gather_shards, resolve_shard, shard_layout


def _f32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


class FlatEMA:
    """``shadow``: fp32 [flat.numel], starts as ``flat.params.float()``; ``num_updates``: the steps taken (a checkpoint's update count
    is assigned to it by the caller, as the reference passes ``get_num_updates()``).
    shard=(rank, world) (either may be None: the process group's): ``shadow`` is fp32 [8 * (S8 + tail8)], this rank's ``[shard | tail]``
    of ``distributed.shard_layout``, and ``layout`` says where it lies; default: the full average, ``layout`` None."""

    def __init__(self, flat: FlatParameters, decay=0.9999, start_update=0, ema_fp32=True, skip_keys=None, shard=None,
                 process_group=None):
        if not ema_fp32:
            raise ValueError("FlatEMA: ema_fp32=False is refused: at decay 0.9999 an average stored in bf16 never moves "
                             "(take * p is below half a bf16 spacing); only the fp32 average is built")
        if skip_keys:
            raise ValueError("FlatEMA: skip_keys is refused: the trainer passes none (trainer.py:250) and the flat update has no "
                             "per-parameter exceptions")
        if not 0.0 <= decay <= 1.0:
            raise ValueError("FlatEMA: decay %r is not in [0, 1]" % (decay,))
        self.flat, self.decay, self.start_update = flat, float(decay), int(start_update)
        self.layout, self.pg = None, process_group
        if shard is not None:
            rank, world = resolve_shard(shard[0], shard[1], process_group)
            self.layout = shard_layout(flat.numel, world, rank)
            self.shadow = self.layout.take(flat.params.detach()).to(torch.float32)  # take() made a new tensor
        else:
            self.shadow = flat.params.detach().to(torch.float32, copy=True)  # an owned copy, also when the parameters are fp32 themselves
        self.num_updates = 0

    # ------------------------------------------------------------------------------------------------------------ the rule
    def decay_at(self, updates):
        return 0.0 if updates < self.start_update else self.decay

    def coefficients(self, updates):
        """(keep, take) of the step that makes ``updates`` the update count, as the fp32 numbers the kernels receive."""
        d = self.decay_at(updates)
        return _f32(d), _f32(1.0 - d)

    @torch.no_grad()
    def step(self, updates=None):
        """One update from ``flat.params`` as they stand (call it after the optimiser step; ``FusedAdamW(ema=...)`` and
        ``TorchAdamW(ema=...)`` do it themselves).  bf16 parameters on the device: one ``hip.ema_step`` launch; anything else: the
        reference's two lines in torch on the flat buffers.  In shard mode: the same on the rank's two ranges, no collective.
        Non-finite values: a NaN parameter (a NaN gradient stepped without clipping) turns exactly its own element of the average
        non-finite.  A step whose clipped gradient norm is NaN makes every parameter NaN (optim.FusedAdamW.step) and with them the
        WHOLE average, fused or not: check the returned norm before stepping, as the reference does (trainer.py:830-837)."""
        updates = self.num_updates + 1 if updates is None else updates
        for shadow, p in self._pairs():
            if p.is_cuda and p.dtype == torch.bfloat16:
                keep, take = self.coefficients(updates)
                hip.ema_step(shadow, p, keep, take)
            else:
                d = self.decay_at(updates)
                shadow.mul_(d)
                shadow.add_(p.to(shadow.dtype), alpha=1.0 - d)
        self.num_updates = updates

    def _pairs(self):
        """[(average, parameters)] as views: the whole buffers, or in shard mode the rank's ranges."""
        if self.layout is None:
            return [(self.shadow, self.flat.params)]
        return [(self.shadow[lo:lo + b - a], self.flat.params[a:b]) for a, b, lo in self.layout.ranges]

    # ------------------------------------------------------------------------------------------------------------ checkpoints
    def full_shadow(self):
        """The fp32 average of the whole buffer: ``shadow`` itself, or in shard mode every rank's part gathered into a new tensor, the
        same on every rank (COLLECTIVE: one all-gather; the tail is replicated)."""
        return self.shadow if self.layout is None else gather_full(self.shadow, self.layout, self.pg)

    def fp32_params(self):
        """name -> fp32 view of the average of that parameter: ``extra_state["ema_fp32_params"]`` (trainer.py:399).  In shard mode
        COLLECTIVE (``full_shadow``), and views of the gathered copy."""
        full = self.full_shadow()
        return OrderedDict((n, full[o:o + k].view(p.shape)) for n, p, o, k in self.flat.entries)

    def ema_state(self, model):
        """An OrderedDict shaped like ``model.state_dict()``: the averaged parameters as the cast of the average to the parameter
        dtype (what the reference's EMA model holds after a step), buffers and frozen parameters from the live model
        (utils/ema_module.py:148-151).  ``extra_state["ema"]`` (trainer.py:396).  In shard mode COLLECTIVE (``full_shadow``)."""
        full = self.full_shadow()
        avg = {n: full[o:o + k].view(p.shape).to(p.dtype, copy=True) for n, p, o, k in self.flat.entries}
        return OrderedDict((key, avg[key] if key in avg else val.detach().clone()) for key, val in model.state_dict().items())

    @torch.no_grad()
    def restore(self, state, fp32_params=None):
        """trainer.py:574-595: per parameter the fp32 value of ``fp32_params`` if it is there, otherwise the value of ``state`` (a
        bf16 EMA model, or the model itself when the checkpoint has no EMA) widened to fp32.  Unknown keys and parameters missing from
        both are skipped, as ``load_state_dict(strict=False)`` does; like it, a tensor of another shape than its parameter raises
        (``ValueError``, before anything is written): a checkpoint of a differently shaped model never restores part of the average.
        In shard mode the full dictionaries are taken as well and only the own ranges are kept; no collective."""
        found = []
        for n, p, o, k in self.flat.entries:
            src = fp32_params.get(n) if fp32_params is not None else None
            if src is None:
                src = state.get(n) if state is not None else None
            if src is None:
                continue
            if not torch.is_tensor(src) or src.shape != p.shape:
                raise ValueError("FlatEMA.restore: %s has shape %s, the parameter %s" % (
                    n, tuple(src.shape) if torch.is_tensor(src) else type(src).__name__, tuple(p.shape)))
            found.append((o, k, src))
        for o, k, src in found:
            src = src.detach().reshape(-1)
            if self.layout is None:
                self.shadow[o:o + k].copy_(src)
                continue
            for a, b, lo in self.layout.ranges:
                x, y = max(a, o), min(b, o + k)
                if y > x:
                    self.shadow[lo + x - a:lo + y - a].copy_(src[x - o:y - o])

    # ------------------------------------------------------------------------------------------------------------ using the average
    def _write_params(self, src):
        """src: a full-length tensor, or None: the average (in shard mode the own ranges, then the gather the optimiser runs)."""
        with torch.no_grad():
            if src is not None or self.layout is None:
                self.flat.params.copy_(self.shadow if src is None else src)  # fp32 -> bf16: round to nearest even
            else:
                for shadow, p in self._pairs():
                    p.copy_(shadow)
                gather_shards(self.flat.params, self.layout, self.pg)
        if self.flat.params.is_cuda:
            ops.refresh_weight_cache()   # the derived copies (transposed weights, fp8) follow the parameters

    @contextlib.contextmanager
    def applied(self):
        """Validation or export with the averaged weights: inside, ``flat.params`` (and with it every model parameter) is the cast of
        the average; on exit the saved parameters (2 B/param) come back bit for bit, also when the body raises.  An optimiser's
        master copy is never touched, so training goes on as if nothing had happened.  In shard mode COLLECTIVE on entry: every
        rank writes the cast of its ranges and the parameters are gathered as after an optimiser step; the exit is local."""
        saved = self.flat.params.detach().clone()
        self._write_params(None)
        try:
            yield self
        finally:
            self._write_params(saved)

    def reverse(self):
        """Write the averaged weights into the parameters for good (utils/ema_module.py:161-171: inference or fine-tuning from the EMA
        model).  An optimiser that keeps a master must be told: call its ``sync_master()`` afterwards.  In shard mode COLLECTIVE."""
        self._write_params(None)
