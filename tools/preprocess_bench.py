"""Image pre-processing of the hub (process_image): host cost vs the HIP path, per batch, in ms.

    python tools/preprocess_bench.py [--size 256] [--out FILE.jsonl]

Cases: COCO-like photos (640 x 480, landscape and portrait mixed), 12 MP photos (4000 x 3000) and thumbnails smaller than S
(160 x 120), at B = 1, 8, 64.  Per case (medians):
  decode_ms        host JPEG decode + .convert("RGB") with PIL (quality-90 JPEGs made here)
  pil_1t_ms        host PIL Image.resize((S, S), BICUBIC) + ToTensor / Normalize in torch, one thread
  pil_16t_ms       the same over a 16-thread pool (PIL releases the GIL while it resizes)
  h2d_ms           the one copy of the packed uint8 buffer (pinned) to the device
  kernel_ms        op_image_resize_normalize alone (both passes, bf16 out), device events
  pack_ms          host pack_images (coefficient tables + copy into the pinned buffer)
Every device result is checked against PIL's (uint8 output) before timing."""
import argparse
import ctypes
import io
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from one_peace_amd import hip, imageprep  # noqa: E402


def images(kind, B, seed):
    g = np.random.default_rng(seed)
    out = []
    for i in range(B):
        if kind == "coco":
            H, W = (480, 640) if i % 3 else (640, 480)
        elif kind == "12mp":
            H, W = (3000, 4000) if i % 2 == 0 else (4000, 3000)
        else:
            H, W = (120, 160) if i % 2 == 0 else (160, 120)
        small = g.integers(0, 256, (H // 8 + 1, W // 8 + 1, 3), dtype=np.uint8)  # blocky content: JPEG-like entropy
        img = np.repeat(np.repeat(small, 8, 0), 8, 1)[:H, :W]
        img = (img.astype(np.int16) + g.integers(-8, 9, img.shape)).clip(0, 255).astype(np.uint8)
        out.append(img)
    return out


def median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def device_ms(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from PIL import Image
    S = args.size
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    pool = ThreadPoolExecutor(16)
    rows = []
    for kind in ("coco", "12mp", "thumb"):
        for B in (int(b) for b in args.batches.split(",")):
            arrs = images(kind, B, seed=B)
            jpegs = []
            for a in arrs:
                f = io.BytesIO()
                Image.fromarray(a).save(f, format="JPEG", quality=90)
                jpegs.append(f.getvalue())
            reps = 3 if kind == "12mp" and B == 64 else 5

            def decode():
                return [Image.open(io.BytesIO(j)).convert("RGB") for j in jpegs]
            pils = decode()

            def host_one(im):
                u8 = torch.from_numpy(np.array(im.resize((S, S), Image.BICUBIC), dtype=np.uint8))
                return imageprep.to_tensor_normalize(u8)

            def host_1t():
                return torch.stack([host_one(im) for im in pils])

            def host_16t():
                return torch.stack(list(pool.map(host_one, pils)))
            decoded = [np.asarray(im) for im in pils]
            t0 = time.perf_counter()
            packed = imageprep.pack_images(decoded, S)
            pack_ms = (time.perf_counter() - t0) * 1e3
            buf = torch.empty(packed.host.numel(), dtype=torch.uint8, device=dev)
            h2d = device_ms(lambda: buf.copy_(packed.host, non_blocking=True), reps=10)
            ws = torch.empty(max(packed.workspace_bytes, 16), dtype=torch.uint8, device=dev)
            out = torch.empty(B, 3, S, S, dtype=torch.bfloat16, device=dev)
            m = (ctypes.c_float * 3)(*imageprep.CLIP_MEAN)
            sd = (ctypes.c_float * 3)(*imageprep.CLIP_STD)
            base = buf.data_ptr()

            def kernel():
                hip._check(hip.lib().op_image_resize_normalize(
                    ctypes.c_void_p(base), packed.src_bytes, ctypes.c_void_p(base + packed.desc_off),
                    packed.desc.ctypes.data_as(ctypes.c_void_p), B, ctypes.c_void_p(base + packed.coef_off), packed.coef_count, S, m, sd,
                    hip.ptr(out), hip.DT_BF16, hip.ptr(ws), ws.numel(), hip.stream()), "op_image_resize_normalize")
            kernel_ms = device_ms(kernel, reps=20)
            ref = host_1t()
            assert torch.equal(out.cpu(), ref.to(torch.bfloat16)), (kind, B)  # device result == PIL + torchvision
            row = {"case": kind, "B": B, "S": S, "src_mb": round(sum(a.nbytes for a in decoded) / 2 ** 20, 2),
                   "decode_ms": round(median_ms(decode, reps), 3), "pil_1t_ms": round(median_ms(host_1t, reps), 3),
                   "pil_16t_ms": round(median_ms(host_16t, reps), 3), "pack_ms": round(pack_ms, 3), "h2d_ms": round(h2d, 4),
                   "kernel_ms": round(kernel_ms, 4), "workspace_mb": round(packed.workspace_bytes / 2 ** 20, 3)}
            print(json.dumps(row), flush=True)
            rows.append(row)
            del buf, ws, out, packed
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
