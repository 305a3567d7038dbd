"""The sharded optimiser state over real collectives: optim.ShardedFusedAdamW (or, with --cpu, optim.ShardedTorchAdamW) with an fp32
master and a sharded ema.FlatEMA on every rank, beside an unsharded twin on deep copies, bit for bit.

    python -m torch.distributed.run --nproc-per-node W tools/sharded_adamw_check.py [--cpu] [--steps 3]

Environment, as tests/test_distributed_gpu.py uses it: ONEPEACE_DIST_BACKEND (gloo: the collectives of W ranks on one device),
ONEPEACE_SINGLE_DEVICE_DEBUG (every rank on device 0), ONEPEACE_FORCE_COLLECTIVES (the collectives also at world 1: the in-place
all-gather over RCCL on a one-GPU box).

Per rank: a small synthetic module with layer-decay groups (`build_module`: sized so that the replicated tail of
distributed.shard_layout is not empty at this world size), FlatParameters, BucketedGradReducer, the sharded optimiser with
master_weights and a sharded EMA; the twin is FusedAdamW / TorchAdamW with master_weights and a full FlatEMA over a deep copy.  Every step
each rank draws its own data, the gradients are all-reduced by the reducer, copied to the twin, and both step with 1 / world and
clipping on.  After every step: parameters, the own ranges of both moments and the master, and the own ranges of the average must equal
the twin's bits.  Then full_shadow() against the twin's shadow, the parameters inside applied() against the twin's and after it against
the saved ones, and a round trip of the average through ema_state() / fp32_params() / restore().  Every rank prints
`sharded check: IDENTICAL` or fails with the first differing index."""
import argparse
import copy
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS, LAYER_DECAY = 3, 0.75
HYPER = dict(lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05)
CLIP_NORM = 0.05  # far below the norm of these gradients: the clip coefficient is active in every step


class Layered(torch.nn.Module):
    """An embedding table, LAYERS x (matrix, bias) and a closing vector of `extra8` vectors: 212 + extra8 vectors in the flat buffer,
    2 * (LAYERS + 1) + 1 groups under `groups_of`.  Elementwise only: the check is about the optimiser, not about GEMMs."""

    def __init__(self, extra8, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        rnd = lambda *shape: torch.nn.Parameter(0.5 * torch.randn(*shape, generator=gen))  # noqa: E731
        self.embed = rnd(50, 8)
        self.weights = torch.nn.ParameterList([rnd(24, 17) for _ in range(LAYERS)])
        self.biases = torch.nn.ParameterList([rnd(17) for _ in range(LAYERS)])
        self.head = rnd(8 * extra8)

    def loss(self, gen):
        """Each parameter against its own random data: a gradient for every element, different for every generator state."""
        total = 0.0
        for p in self.parameters():
            x = torch.randn(p.shape, generator=gen).to(p.device, p.dtype)
            total = total + torch.tanh(p * x).float().sum()
        return total


def build_module(worlds, seed=0):
    """Layered with the smallest closing vector (>= 1) that leaves a non-empty tail at every world size > 1 in `worlds`."""
    base8 = 50 + LAYERS * (51 + 3)
    extra8 = next(e for e in range(1, 1000) if all((base8 + e) % w for w in worlds if w > 1))
    return Layered(extra8, seed)


def groups_of(model):
    """(no_decay, lr_scale) for FlatParameters: biases and the head undecayed, lr scaled by LAYER_DECAY per layer from the top."""
    def layer(name):
        return 0 if name.startswith("embed") else (LAYERS + 1 if name.startswith("head") else int(name.split(".")[1]) + 1)
    return (lambda name, p: p.ndim <= 1), (lambda name, p: LAYER_DECAY ** (LAYERS + 1 - layer(name)))


def first_difference(a, b):
    """None when a and b hold the same bits, otherwise the first index at which they differ."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return "shape/dtype %s %s against %s %s" % (tuple(a.shape), a.dtype, tuple(b.shape), b.dtype)
    view = torch.int16 if a.element_size() == 2 else torch.int32
    diff = (a.detach().contiguous().view(view) != b.detach().contiguous().view(view)).nonzero()
    return None if diff.numel() == 0 else int(diff[0])


def run(args):
    from one_peace_amd.distributed import BucketedGradReducer, FlatParameters, init_distributed
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd import optim
    backend = "gloo" if args.cpu else os.environ.get("ONEPEACE_DIST_BACKEND")
    if args.cpu:
        os.environ.setdefault("ONEPEACE_SINGLE_DEVICE_DEBUG", "1")  # no rank selects a device of its own
    rank, world, local = init_distributed(backend)
    if args.cpu:
        device, sharded_cls, twin_cls = torch.device("cpu"), optim.ShardedTorchAdamW, optim.TorchAdamW
    else:
        if not torch.cuda.is_available():
            sys.exit("sharded_adamw_check: no GPU (use --cpu for the torch classes over gloo)")
        device = torch.device("cuda", 0 if os.environ.get("ONEPEACE_SINGLE_DEVICE_DEBUG") else local)
        torch.cuda.set_device(device)
        sharded_cls, twin_cls = optim.ShardedFusedAdamW, optim.FusedAdamW

    def must_match(what, got, want):
        at = first_difference(got, want)
        if at is not None:
            sys.exit("[rank %d] sharded check: %s DIFFERS from the unsharded twin, first at index %s" % (rank, what, at))

    model = build_module((world,)).to(device).to(torch.bfloat16)  # the same seed on every rank: replicas start identical
    twin_model = copy.deepcopy(model)
    flat = FlatParameters(model, *groups_of(model))
    twin_flat = FlatParameters(twin_model, *groups_of(twin_model))
    reducer = BucketedGradReducer(flat, bucket_bytes=1024)
    ema = FlatEMA(flat, decay=0.9, start_update=2, shard=(rank, world))
    opt = sharded_cls(flat, master_weights=True, ema=ema, **HYPER)
    twin_ema = FlatEMA(twin_flat, decay=0.9, start_update=2)
    twin = twin_cls(twin_flat, master_weights=True, ema=twin_ema, **HYPER)
    lay = opt.layout
    assert (lay.rank, lay.world) == (rank, world) and (world == 1 or lay.tail8 > 0), lay
    assert opt.exp_avg.numel() == lay.local_numel and opt.state_bytes() == 16 * lay.local_numel

    gen = torch.Generator().manual_seed(1234 + rank)  # different data on every rank
    for step in range(1, args.steps + 1):
        opt.zero_grad()
        reducer.reset()
        model.loss(gen).backward()
        reducer.finish()
        twin_flat.grads.copy_(flat.grads)
        norm = opt.step(grad_scale=1.0 / world, clip_norm=CLIP_NORM)
        twin_norm = twin.step(grad_scale=1.0 / world, clip_norm=CLIP_NORM)
        assert float(norm) > 10 * CLIP_NORM, "step %d: the norm %g does not clip" % (step, float(norm))
        must_match("step %d norm" % step, norm.reshape(1), twin_norm.reshape(1))
        must_match("step %d params" % step, flat.params, twin_flat.params)
        for name, got, want in (("exp_avg", opt.exp_avg, twin.exp_avg), ("exp_avg_sq", opt.exp_avg_sq, twin.exp_avg_sq),
                                ("master", opt.master, twin.master), ("ema", ema.shadow, twin_ema.shadow)):
            must_match("step %d %s (own ranges)" % (step, name), got, lay.take(want))
    assert ema.num_updates == twin_ema.num_updates == args.steps

    must_match("full_shadow", ema.full_shadow(), twin_ema.shadow)
    saved = flat.params.clone()
    with ema.applied(), twin_ema.applied():
        must_match("params inside applied()", flat.params, twin_flat.params)
        assert first_difference(flat.params, saved) is not None, "applied() left the parameters as they were"
    must_match("params after applied()", flat.params, saved)
    state, fp32 = ema.ema_state(model), ema.fp32_params()
    for n, want in twin_ema.fp32_params().items():
        must_match("fp32_params[%s]" % n, fp32[n], want)
    other = FlatEMA(flat, decay=0.9, shard=(rank, world))
    other.shadow.zero_()
    other.restore(state, fp32)
    padding = torch.ones(flat.numel, dtype=torch.bool, device=device)  # the alignment gaps between parameters belong to no entry
    for _, _, o, k in flat.entries:
        padding[o:o + k] = False
    must_match("restore(ema_state, fp32_params)", other.shadow, lay.take(torch.where(padding, 0.0, twin_ema.shadow)))
    other.restore(state)
    must_match("restore(ema_state)", other.shadow,
               lay.take(torch.where(padding, 0.0, twin_ema.shadow.to(torch.bfloat16).float())))
    if not args.cpu:
        torch.cuda.synchronize()
    print("[rank %d of %d, %s, %s] sharded check: IDENTICAL\n" % (rank, world, device, sharded_cls.__name__), end="", flush=True)
    import torch.distributed as dist
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cpu", action="store_true", help="the torch classes on the CPU over gloo")
    ap.add_argument("--steps", type=int, default=3)
    run(ap.parse_args())


if __name__ == "__main__":
    main()
