"""Fine-tuning criteria on the device: the HIP route (ops.classify_loss / ops.hinge_loss / ops.box_loss over csrc/losses.hip) against the
torch statement of the same criterion (the reference's own calls; the GIoU diagonal written out), forward + backward.

    python tools/criteria_bench.py [--iters 200] [--rounds 7] [--out FILE]

Shapes: the (B, C) of the reference's fine-tuning YAMLs -- vqa 8 x 3129 (multi-label), fsd50k 8 x 200 (multi-label), vggsound 8 x 309,
nlvr2 8 x 2, image classification x 1000 (no YAML ships for it: B = 64, label smoothing 0.1), aqa 1 x 4 choices (hinge),
visual grounding 4 boxes -- and the same heads at B = 128, since the shipped batches are per-GPU micro-batches.  bf16 logits, as the
heads produce them.

Method: device events around `iters` forward + backward calls, every shape warmed up first, the two routes alternating round by round
in one process; the median over the rounds, and their spread, in microseconds per call.  Launches per call are counted in a separate,
untimed pass with the profiler (kernels of any origin on the device).  There is no CPU mode: without a device the tool fails."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_route(kind, logits, targets, eps):
    if kind == "multi":
        return F.binary_cross_entropy_with_logits(logits, targets, reduction="sum"), targets.gather(1, logits.argmax(1, keepdim=True)).sum()
    if kind == "soft":
        lp = F.log_softmax(logits, dim=-1, dtype=torch.float32)
        return (-targets * lp).sum(), (lp.exp() * targets).sum().detach()
    if kind == "hard":
        return F.cross_entropy(logits, targets, label_smoothing=eps, reduction="sum"), logits.argmax(1).eq(targets).sum()
    if kind == "hinge":
        pos = logits.gather(1, targets.unsqueeze(1))
        return torch.max(torch.tensor(0.0, device=logits.device), 1 + logits - pos).sum(), logits.argmax(1).eq(targets).sum()
    from one_peace_amd.ops import box_loss_torch
    return box_loss_torch(logits, targets), None


def hip_route(kind, logits, targets, eps):
    from one_peace_amd import ops
    if kind == "hinge":
        return ops.hinge_loss(logits, targets, 1.0)
    if kind == "box":
        return ops.box_loss(logits, targets), None
    return ops.classify_loss(logits, targets, use_multi_label=kind == "multi", label_smoothing=eps)


def make(kind, B, C, dev):
    g = torch.Generator().manual_seed(B * 7919 + C)
    x = (torch.randn(B, C, generator=g) * 4).to(dev, torch.bfloat16)
    if kind == "multi":
        t = (torch.rand(B, C, generator=g) < 0.01).to(dev, torch.bfloat16)
    elif kind == "soft":
        t = (torch.rand(B, C, generator=g) * (torch.rand(B, C, generator=g) < 0.01)).to(dev, torch.float32)
    elif kind == "box":
        lo = 0.1 + 0.4 * torch.rand(B, 2, generator=g)
        t = torch.cat([lo, lo + 0.1 + 0.3 * torch.rand(B, 2, generator=g)], 1).to(dev)
        x = (torch.randn(B, 4, generator=g) + torch.tensor([-1.0, -1.0, 1.0, 1.0])).to(dev, torch.bfloat16)
    else:
        t = torch.randint(0, C, (B,), generator=g).to(dev)
    return x.requires_grad_(True), t


def step(route, kind, x, t, eps):
    x.grad = None
    loss, _ = route(kind, x, t, eps)
    loss.backward()


def timed(route, kind, x, t, eps, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        step(route, kind, x, t, eps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters


def launches(route, kind, x, t, eps):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step(route, kind, x, t, eps)
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA") and "memcpy" not in e.name.lower())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("criteria_bench: no GPU; this tool measures on the device only")
    import one_peace_amd  # noqa: F401
    dev = "cuda"
    shapes = [("vqa", "multi", 8, 3129, 0.0), ("fsd50k", "multi", 8, 200, 0.0), ("vggsound", "hard", 8, 309, 0.0), ("nlvr2", "hard", 8, 2, 0.0),
              ("image_classify", "hard", 64, 1000, 0.1), ("vqa_soft", "soft", 8, 3129, 0.0), ("aqa", "hinge", 1, 4, 0.0),
              ("visual_grounding", "box", 4, 4, 0.0),
              ("vqa_b128", "multi", 128, 3129, 0.0), ("vggsound_b128", "hard", 128, 309, 0.0), ("image_classify_b128", "hard", 128, 1000, 0.1),
              ("aqa_b128", "hinge", 128, 4, 0.0), ("visual_grounding_b128", "box", 128, 4, 0.0)]
    lines = []
    print("device:", torch.cuda.get_device_name(0), "| torch", torch.__version__, "| iters", args.iters, "rounds", args.rounds)
    for name, kind, B, C, eps in shapes:
        x, t = make(kind, B, C, dev)
        for route in (hip_route, torch_route):
            for _ in range(20):
                step(route, kind, x, t, eps)
        torch.cuda.synchronize()
        res = {"hip": [], "torch": []}
        for _ in range(args.rounds):
            res["hip"].append(timed(hip_route, kind, x, t, eps, args.iters))
            res["torch"].append(timed(torch_route, kind, x, t, eps, args.iters))
        try:
            n_hip, n_torch = launches(hip_route, kind, x, t, eps), launches(torch_route, kind, x, t, eps)
        except Exception as e:  # the count is a side product; the timings stand without it
            n_hip = n_torch = "n/a (%s)" % type(e).__name__
        row = {"case": name, "kind": kind, "B": B, "C": C, "label_smoothing": eps,
               "hip_us": round(statistics.median(res["hip"]), 2), "hip_us_min_max": [round(min(res["hip"]), 2), round(max(res["hip"]), 2)],
               "torch_us": round(statistics.median(res["torch"]), 2), "torch_us_min_max": [round(min(res["torch"]), 2), round(max(res["torch"]), 2)],
               "torch_over_hip": round(statistics.median(res["torch"]) / statistics.median(res["hip"]), 3),
               "launches_hip": n_hip, "launches_torch": n_torch}
        lines.append(json.dumps(row))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
