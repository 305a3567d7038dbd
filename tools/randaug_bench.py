"""RandAugment and RandomErasing at the fine-tuning batch: the device routes (op_image_randaug_layer, op_image_color_jitter for the
ImageEnhance blends, op_image_erase) against the same work in Pillow / torch on one host thread.

    python tools/randaug_bench.py [--batch 128] [--size 256] [--legs 5] [--reps 20] [--out profiles/randaug_mi355x.json]

Three groups of rows:
  op:<name>         every image of the uint8 [B, S, S, 3] batch gets that one op (ops.rand_augment with a one-layer table), largest magnitude
  randaug_drawn     a drawn 'rand-m9-mstd0.5-inc1' batch (two layers); erase: RandomErasing(0.25, 'pixel') boxes through ops.erase_images on
                    the normalised bf16 batch; create_transform: the whole call from decoded images to the erased bf16 batch
  each beside the same work on the host (Pillow per image, one thread, wall clock over the batch) and beside algorithmic bytes over the
  call time: a pointwise op reads and writes the image (2 x), a histogram op and Contrast read it once more (3 x), Sharpness and the
  affine ops read it, write the scratch and copy it back (4 x); the erase reads 4 and writes 2 bytes per erased element.
Device times: `legs` legs of `reps` calls between two device events, medians over the legs with their spread; the tables' host-to-device
copy is part of every call, as in the product path.  Before timing, the device result of every op is compared with Pillow's byte for
byte on the first images."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from one_peace_amd import augment, hip, imageprep, ops  # noqa: E402

PASSES = {0: 0, 1: 3, 2: 3, 3: 2, 4: 2, 5: 2, 6: 2, 7: 2, 8: 3, 9: 2, 10: 4, 11: 4}  # times the image's bytes move, by op code


def leg_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def measure(fn, legs, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = [leg_ms(fn, reps) for _ in range(legs)]
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("randaug_bench: needs a GPU (nothing is measured without one)")
    hip.lib()
    torch.set_num_threads(1)
    B, S = a.batch, a.size
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    src = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
    fill = augment.RandAugment().fill
    img_bytes = S * S * 3
    rows = []

    def add(row, fn, nbytes, host_fn):
        row.update({"B": B, "S": S, "algorithmic_bytes": int(nbytes)})
        row.update(measure(fn, a.legs, a.reps))
        row["GBps"] = nbytes / (row["median_ms"] * 1e-3) / 1e9
        row["host_ms_one_thread"] = host_ms(host_fn)
        row["host_over_device"] = row["host_ms_one_thread"] / row["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)

    def table_bytes(tab_ops):
        return sum(PASSES[int(o)] for o in tab_ops.reshape(-1)) * img_bytes

    # ---- one op kind on every image ----
    items = [("AutoContrast",), ("Equalize",), ("Invert",), ("Posterize", 0), ("Solarize", 26), ("SolarizeAdd", 99), ("Color", 1.9),
             ("Contrast", 1.9), ("Brightness", 1.9), ("Sharpness", 1.9), ("Rotate", 30.0), ("ShearX", 0.3), ("TranslateX", 0.45 * S)]
    for item in items:
        tab = imageprep.randaug_table([[item]] * B, S)
        u8 = src.to(dev)
        ops.rand_augment(u8, *tab, fill)
        want = ops.rand_augment(src[:4].clone(), tab[0][:4], tab[1][:4], fill)
        assert torch.equal(u8[:4].cpu(), want), "the device result of %s differs from Pillow's" % (item,)
        add({"case": "op:" + item[0]}, lambda: ops.rand_augment(u8, *tab, fill), table_bytes(tab[0]),
            lambda: ops.rand_augment(src.clone(), *tab, fill))

    # ---- a drawn rand-m9-mstd0.5-inc1 batch ----
    tab = augment.RandAugment.from_config("rand-m9-mstd0.5-inc1", generator=g).params(B, S)
    u8 = src.to(dev)
    ops.rand_augment(u8, *tab)
    assert torch.equal(u8.cpu(), ops.rand_augment(src.clone(), *tab)), "the drawn batch differs from Pillow's"
    add({"case": "randaug_drawn", "config": "rand-m9-mstd0.5-inc1", "ops_applied": int((tab[0] != 0).sum())}, lambda: ops.rand_augment(u8, *tab),
        table_bytes(tab[0]), lambda: ops.rand_augment(src.clone(), *tab))

    # ---- the erase launch ----
    er = augment.RandomErasing(0.25, mode="pixel", generator=g)
    boxes = er.params(B, S, S)
    x = torch.randn(B, 3, S, S, generator=g).to(torch.bfloat16)
    x_dev, noise = x.to(dev), er.noise(boxes, torch.device("cpu"))
    noise_dev = noise.to(dev)
    assert torch.equal(ops.erase_images(x_dev, boxes, noise_dev).cpu(), ops.erase_images(x.clone(), boxes, noise)), "the erase differs from torch's"
    add({"case": "erase_bf16", "erased_images": int((boxes[:, 2] > 0).sum())}, lambda: ops.erase_images(x_dev, boxes, noise_dev), noise.numel() * 6,
        lambda: ops.erase_images(x.clone(), boxes, noise))

    # ---- the whole create_transform call, from decoded images ----
    images = [torch.randint(0, 256, (320 + 8 * (i % 9), 400 - 8 * (i % 7), 3), generator=g, dtype=torch.uint8).numpy() for i in range(B)]
    make = lambda: augment.create_transform(S, True, 0.4, "rand-m9-mstd0.5-inc1", "bicubic", re_prob=0.25, re_mode="pixel", re_count=1,
                                            generator=torch.Generator().manual_seed(1))
    assert torch.equal(make()(images, torch.bfloat16, dev).cpu(), make()(images, torch.bfloat16, "cpu")), "create_transform: device != host"
    t_dev, t_host = make(), make()
    src_bytes = sum(im.size for im in images)
    add({"case": "create_transform_bf16", "source_bytes": int(src_bytes)}, lambda: t_dev(images, torch.bfloat16, dev),
        src_bytes + B * img_bytes * (1 + 2 * 3 + 1 + 2), lambda: t_host(images, torch.bfloat16, "cpu"))

    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "legs": a.legs, "reps_per_leg": a.reps, "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
