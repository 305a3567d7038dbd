"""Device augmentation at the fine-tuning batch: Mixup / CutMix in op_mix_images against the torch statement, and the flip entry of the
resize pass against the plain entry.

    python tools/augment_bench.py [--batch 128] [--size 256] [--legs 5] [--reps 50] [--out profiles/augment_mi355x.json]

Mix, per dtype (fp32, bf16) and kind (Mixup, CutMix; per-element tables): op_mix_images IN PLACE against the reference's torch
statement on the same device -- x.mul_(lam).add_(x.flip(0).mul_(1 - lam)) for Mixup, x[:, :, yl:yh, xl:xh] = x.flip(0)[...] for CutMix
(timm's batch-mode statements; ONE box for the batch, which is the cheapest torch can do) -- in alternating legs of `reps` calls each,
timed with device events around a leg; the medians over the legs are reported with their spread (min ... max).  Rates are algorithmic
bytes, B * 3 * S^2 * (input + output bytes), over the call time.  Before timing the kernel's output is compared with the statement's
(bit for bit in fp32).
Flip: op_image_resize_normalize_flip with every image flipped against op_image_resize_normalize on the same packed batch of 640 x 480
images (bf16 out), same alternation; the ratio of the medians is recorded."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from one_peace_amd import augment, hip, imageprep  # noqa: E402


def leg_ms(fn, reps):
    """ms per call of `reps` back-to-back calls between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def alternate(fns, legs, reps, warmup=10):
    """{name: [ms per call of each leg]} with the candidates taking turns (A B A B ...), every one warmed up first."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(legs):
        for k, fn in fns.items():
            out[k].append(leg_ms(fn, reps))
    return out


def summary(ms):
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def bench_mix(B, S, dtype, kind, legs, reps):
    dev = torch.device("cuda", torch.cuda.current_device())
    x = torch.randn(B, 3, S, S, device=dev).to(dtype)
    np.random.seed(0)
    m = augment.Mixup(mixup_alpha=0.8 if kind == "mixup" else 0.0, cutmix_alpha=0.0 if kind == "mixup" else 1.0, mode="batch")
    params, lam = m._draw(B, S, S)  # batch mode: lam is the Python double timm keeps, the tables hold fl32(lam) and fl32(1 - lam)
    box = [int(v) for v in params[3][0]]
    tables = hip.mix_tables(params, B, dev)

    def torch_statement(t):
        if kind == "mixup":
            x_flipped = t.flip(0).mul_(1.0 - lam)
            return t.mul_(lam).add_(x_flipped)
        yl, yh, xl, xh = box
        t[:, :, yl:yh, xl:xh] = t.flip(0)[:, :, yl:yh, xl:xh]
        return t

    if dtype == torch.float32:  # the check: in place, bit for bit (bf16: torch rounds three times, the kernel once -- not comparable)
        want, got = torch_statement(x.clone()), x.clone()
        assert hip.mix_images(got, tables, got) is got and torch.equal(got, want), "op_mix_images differs from the torch statement"
    y, z = x.clone(), x.clone()
    ms = alternate({"hip": lambda: hip.mix_images(y, tables, y), "torch": lambda: torch_statement(z)}, legs, reps)
    nbytes = B * 3 * S * S * 2 * x.element_size()
    row = {"case": "mix", "kind": kind, "dtype": str(dtype).replace("torch.", ""), "B": B, "S": S, "algorithmic_bytes": nbytes,
           "lam": lam, "box": box}
    for k, v in ms.items():
        row[k] = summary(v)
        row[k]["GBps"] = nbytes / (row[k]["median_ms"] * 1e-3) / 1e9
    row["torch_over_hip"] = row["torch"]["median_ms"] / row["hip"]["median_ms"]
    return row


def bench_flip(B, S, legs, reps):
    dev = torch.device("cuda", torch.cuda.current_device())
    g = np.random.default_rng(1)
    imgs = [g.integers(0, 256, ((480, 640) if i % 3 else (640, 480)) + (3,), dtype=np.uint8) for i in range(B)]
    packed = imageprep.pack_images(imgs, S, flips=[True] * B)
    buf = packed.host.to(dev)
    ws = torch.empty(packed.workspace_bytes, dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, S, S, dtype=torch.bfloat16, device=dev)
    base = buf.data_ptr()
    m, s = (ctypes.c_float * 3)(*imageprep.CLIP_MEAN), (ctypes.c_float * 3)(*imageprep.CLIP_STD)
    args = (ctypes.c_void_p(base), packed.src_bytes, ctypes.c_void_p(base + packed.desc_off), packed.desc.ctypes.data_as(ctypes.c_void_p), B,
            ctypes.c_void_p(base + packed.coef_off), packed.coef_count, S, m, s, hip.ptr(out), hip.DT_BF16, hip.ptr(ws), ws.numel())

    def plain():
        hip._check(hip.lib().op_image_resize_normalize(*args, hip.stream()), "op_image_resize_normalize")

    def flip():
        hip._check(hip.lib().op_image_resize_normalize_flip(*args, ctypes.c_void_p(base + packed.flip_off), hip.stream()),
                   "op_image_resize_normalize_flip")

    plain()
    ref = out.clone()
    flip()
    assert torch.equal(out, ref.flip(3)), "the flip entry is not the mirrored plain entry"
    ms = alternate({"plain": plain, "flip": flip}, legs, reps)
    row = {"case": "flip", "B": B, "S": S, "source": "640 x 480 / 480 x 640 uint8", "dtype": "bfloat16"}
    for k, v in ms.items():
        row[k] = summary(v)
    row["flip_over_plain"] = row["flip"]["median_ms"] / row["plain"]["median_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_bench: needs a GPU (nothing is measured without one)")
    hip.lib()
    rows = []
    for dtype in (torch.float32, torch.bfloat16):
        for kind in ("mixup", "cutmix"):
            rows.append(bench_mix(a.batch, a.size, dtype, kind, a.legs, a.reps))
            print(json.dumps(rows[-1]), flush=True)
    rows.append(bench_flip(a.batch, a.size, a.legs, a.reps))
    print(json.dumps(rows[-1]), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "legs": a.legs, "reps_per_leg": a.reps, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
