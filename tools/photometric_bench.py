"""Photometric train transforms at the fine-tuning batch: the device chain (op_image_color_jitter, op_image_gaussian_blur,
op_image_normalize_flip on the resized uint8 batch) against the same chain in PIL on the host.

    python tools/photometric_bench.py [--batch 128] [--size 256] [--legs 5] [--reps 50] [--out profiles/photometric_mi355x.json]

The batch is uint8 [B, S, S, 3] on the device, as the resize writes it.  Every image gets the NLVR2 / raw_transform steps
(RandomDistortion(0.4, 0.4, 0.4, 0, 0.5) and GaussianBlur(0.5) with both drawn as "applied": three enhancers in a random order, a radius in
[0.1, 2.0]) and a flip flag.  Device: each entry is timed on its own and the three together, `legs` legs of `reps` calls between two device
events, medians over the legs with their spread; the per-launch time is the entry's time over its launches (jitter: the L sum and the
chain; blur: rows and columns; normalize: one), the rate is algorithmic bytes (each launch reads the batch once, the in-place ones write it
once, normalize writes B x 3 x S x S elements) over the time.  The tables' host-to-device copy is part of each call, as in the product path.
Host: ImageEnhance x 3, ImageFilter.GaussianBlur, transpose and the torch ToTensor / Normalize per image, one thread, wall clock over the
batch.  Before timing, the device result is compared with PIL's bit for bit."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from one_peace_amd import augment, hip, imageprep, ops  # noqa: E402


def leg_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(fn, legs, reps, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [leg_ms(fn, reps) for _ in range(legs)]
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def pil_chain(a, ops_row, f_row, radius, flip):
    from PIL import Image
    im = ops._pil_jitter(Image.fromarray(a), ops_row, f_row)
    im = ops._pil_blur(im, radius)
    if flip:
        im = im.transpose(Image.FLIP_LEFT_RIGHT)
    return np.array(im, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("photometric_bench: needs a GPU (nothing is measured without one)")
    hip.lib()
    B, S = a.batch, a.size
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
    jitter = augment.ColorJitter(0.4, 0.4, 0.4, prob=1.0, generator=g).params(B)
    radii = augment.GaussianBlur(p=1.0, generator=g).params(B)
    blur = imageprep.blur_table(radii)
    flips = (torch.rand(B, generator=g) < 0.5).tolist()
    flips_dev = torch.tensor(flips, dtype=torch.uint8).to(dev)
    mean, std = imageprep.CLIP_MEAN, imageprep.CLIP_STD

    # the check: the device chain equals PIL's on the first images, bit for bit
    u8 = src.to(dev)
    hip.image_color_jitter(u8, *jitter)
    hip.image_gaussian_blur(u8, *blur)
    x = hip.image_normalize_flip(u8, mean, std, torch.float32, flips_dev)
    for i in range(min(B, 8)):
        want = pil_chain(src[i].numpy(), jitter[0][i], jitter[1][i], radii[i], flips[i])
        assert torch.equal(x[i].cpu(), imageprep.to_tensor_normalize(torch.from_numpy(want))), "the device chain differs from PIL at image %d" % i

    px = B * S * S * 3
    cases = {
        "color_jitter": (lambda: hip.image_color_jitter(u8, *jitter), 2, 3 * px),
        "gaussian_blur": (lambda: hip.image_gaussian_blur(u8, *blur), 2, 4 * px),
        "normalize_flip_bf16": (lambda: hip.image_normalize_flip(u8, mean, std, torch.bfloat16, flips_dev), 1, px + 2 * px),
        "normalize_flip_fp32": (lambda: hip.image_normalize_flip(u8, mean, std, torch.float32, flips_dev), 1, px + 4 * px),
    }

    def chain():
        hip.image_color_jitter(u8, *jitter)
        hip.image_gaussian_blur(u8, *blur)
        return hip.image_normalize_flip(u8, mean, std, torch.bfloat16, flips_dev)

    cases["chain_bf16"] = (chain, 5, (3 + 4 + 3) * px)
    rows = []
    for name, (fn, launches, nbytes) in cases.items():
        row = {"case": name, "B": B, "S": S, "launches": launches, "algorithmic_bytes": nbytes}
        row.update(measure(fn, a.legs, a.reps))
        row["per_launch_us"] = row["median_ms"] * 1e3 / launches
        row["GBps"] = nbytes / (row["median_ms"] * 1e-3) / 1e9
        rows.append(row)
        print(json.dumps(row), flush=True)

    host = []
    for _ in range(a.host_reps):
        t0 = time.perf_counter()
        for i in range(B):
            imageprep.to_tensor_normalize(torch.from_numpy(pil_chain(src[i].numpy(), jitter[0][i], jitter[1][i], radii[i], flips[i])), mean, std)
        host.append((time.perf_counter() - t0) * 1e3)
    row = {"case": "pil_chain_host", "B": B, "S": S, "threads": 1, "median_ms": float(np.median(host)), "min_ms": float(min(host)),
           "max_ms": float(max(host))}
    row["host_over_device_chain"] = row["median_ms"] / rows[-1]["median_ms"]
    rows.append(row)
    print(json.dumps(row), flush=True)
    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "legs": a.legs, "reps_per_leg": a.reps, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
