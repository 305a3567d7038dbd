"""Audio pre-processing of the hub (process_audio): host cost vs the HIP path, per batch, in ms.

    python tools/audioprep_bench.py [--batches 1,8,64] [--commit ID] [--out FILE.jsonl]
    python tools/audioprep_bench.py --resample [--commit ID] [--out FILE.json]

Cases: mono clips of 1 s, 5 s, 15 s and 60 s (cropped to 15 s) at 16 kHz, int16 PCM and fp32 sources, B = 1, 8, 64, bf16 output (the
hub's dtype).  Per case (medians):
  host_1t_ms    the host route (audioprep.postprocess per clip: layer norm, crop, tile; then the padding loop into fp32 [B, T]), one thread
  host_16t_ms   the same with the clips spread over a 16-thread pool (one clip's layer norm is a single row: torch does not split it)
  h2d_fp32_ms   the copy of that fp32 [B, T] batch to the device, which the host route needs
  pack_ms       host pack_clips (copy into the pinned buffer + descriptor table)
  h2d_ms        the one copy of the packed buffer (pinned) to the device
  kernel_ms     op_audio_normalize_pad alone (both launches), device events
  kernel_gbps   bytes the statistics pass reads (whole clips) + bytes the normalise pass reads (up to the crop) + bytes written, over kernel_ms
  copy_gbps     a torch device-to-device copy that moves the same byte count (half read, half written), timed in the same process
Every device result is checked against the fp64 oracle (the bound of tests/test_audioprep_gpu.py, every element) before timing.
The first line of the output file holds the date, the commit and the device.

--resample: 64 clips of 15 s, int16 stereo at 44.1 kHz, to 16 kHz (ops.resample_audio / ops.preprocess_audio(resample=True)); one record:
  kernel_ms         op_audio_resample alone, device events; kernel_gfma_s = outputs x taps per row (376) over it
  device_route_ms   ops.preprocess_audio(resample=True) on the device end to end: staging, the one H2D copy, both ops, synchronise
  cpu_route_ms      ops.resample_audio on the CPU (fp64 polyphase matrix products): 8 clips timed, scaled to the 64
  scipy_ms          scipy.signal.resample_poly(x, L, M, window=h) on the fp64 mono clips, the same way, where scipy imports (else null)
Clip 0 is checked against the fp64 oracle of tests/audioresample_ref.py (every 97th output, the bound of tests/test_audioresample_gpu.py)
before timing."""
import argparse
import ctypes
import datetime
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from one_peace_amd import audioprep, hip  # noqa: E402

RATE = 16000
MAX_LEN, MIN_LEN = 15 * RATE, RATE


def clips(seconds, fmt, B, seed):
    g = np.random.default_rng(seed)
    out = []
    for i in range(B):
        n = int(seconds * RATE) - 37 * (i % 5)  # lengths differ a little, as decoded files do
        x = 0.02 + 0.3 * g.standard_normal(n).clip(-3, 3) / 3
        out.append(np.round(x * 32768).astype(np.int16) if fmt == "int16" else x.astype(np.float32))
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


def check(out, arrs, dtype):
    """Every element within the derived bound of the fp64 result: B = 2^-24 (4 |y| + 2 |m| r), for bf16 2^-8 (|y| + B) + B."""
    worst = 0.0
    for i, a in enumerate(arrs):
        x = torch.from_numpy(a.astype(np.float32) / 32768.0 if a.dtype == np.int16 else a).double()
        m = x.mean()
        r = 1.0 / torch.sqrt(((x - m) ** 2).mean() + 1e-5)
        y = ((x - m) * r)[:MAX_LEN]
        if y.numel() < MIN_LEN:
            y = y.repeat(-(-MIN_LEN // y.numel()))[:MIN_LEN]
        bound = 2.0 ** -24 * (4 * y.abs() + 2 * abs(float(m)) * float(r))
        if dtype == torch.bfloat16:
            bound = 2.0 ** -8 * (y.abs() + bound) + bound
        got = out[i].double()
        err = (got[: y.numel()] - y).abs()
        assert bool((err <= bound).all()) and int((got[y.numel():] != 0).sum()) == 0, "clip %d misses the bound" % i
        worst = max(worst, float((err / bound).max()))
    return worst


def resample_leg(args, dev):
    from one_peace_amd import ops
    from tests import audioresample_ref as R
    B, rate, seconds = 64, 44100, 15
    g = np.random.default_rng(64)
    arrs = [np.round(0.3 * g.standard_normal((rate * seconds - 37 * (i % 5), 2)).clip(-3, 3) / 3 * 32768).astype(np.int16) for i in range(B)]
    rates = [rate] * B
    packed = audioprep.pack_resample(arrs, rates)
    wavs = hip.audio_resample(packed, dev)
    torch.cuda.synchronize()
    rows = np.arange(0, packed.lengths[0], 97)
    y64, S = R.oracle(arrs[0], rate, rows=rows)
    worst = R.worst_ratio(wavs[0].cpu().numpy()[rows], y64, R.bound(S, rate))
    assert worst <= 1.0, "clip 0 misses the bound: %.3f" % worst
    buf = torch.empty(packed.total_bytes, dtype=torch.uint8, device=dev)
    buf[:packed.host.numel()].copy_(packed.host)
    out = torch.zeros(B, packed.rows, dtype=torch.float32, device=dev)
    base = buf.data_ptr()

    def kernel():
        hip._check(hip.lib().op_audio_resample(
            ctypes.c_void_p(base), packed.src_bytes, ctypes.c_void_p(base + packed.desc_off), packed.desc.ctypes.data_as(ctypes.c_void_p),
            B, ctypes.c_void_p(base + packed.coef_off), packed.coef_count, hip.ptr(out), packed.out_bytes, hip.stream()), "op_audio_resample")
    kernel_ms = device_ms(kernel, reps=20)
    assert torch.equal(out, wavs)
    items = list(zip(arrs, rates))

    def device_route():
        w, _ = ops.preprocess_audio(items, RATE, 15, 1, dtype=torch.bfloat16, device=dev, resample=True)
        torch.cuda.synchronize()
        return w
    device_route()
    device_route_ms = median_ms(device_route, 5)
    pack_ms = median_ms(lambda: audioprep.pack_resample(arrs, rates, norm=(MAX_LEN, MIN_LEN)), 5)
    timed = 8  # clips timed on the host, scaled to the batch
    cpu_ms = median_ms(lambda: ops.resample_audio(arrs[:timed], rates[:timed]), 1) * (B / timed)
    try:
        from scipy import signal
        L, M, h = audioprep.resample_filter(rate)
        mono = [audioprep.mono64(a) for a in arrs[:timed]]
        scipy_ms = median_ms(lambda: [signal.resample_poly(x, L, M, window=h) for x in mono], 1) * (B / timed)
    except ImportError:
        scipy_ms = None
    fma = sum(packed.lengths) * 376
    row = {"tool": "tools/audioprep_bench.py --resample", "date": datetime.date.today().isoformat(), "commit": args.commit,
           "device": torch.cuda.get_device_name(dev), "B": B, "seconds": seconds, "src": "int16 stereo", "rate": rate, "to": RATE,
           "outputs": sum(packed.lengths), "taps_per_row": 376, "h2d_mb": round(packed.host.numel() / 2 ** 20, 1),
           "kernel_ms": round(kernel_ms, 4), "kernel_gfma_s": round(fma / kernel_ms / 1e6, 1), "pack_ms": round(pack_ms, 2),
           "device_route_ms": round(device_route_ms, 2), "host_clips_timed": timed, "cpu_route_ms": round(cpu_ms, 1),
           "scipy_ms": None if scipy_ms is None else round(scipy_ms, 1), "worst_err_over_bound": round(worst, 4)}
    print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(row, indent=1) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--resample", action="store_true", help="the sample-rate conversion leg: 64 clips of 15 s, int16 stereo at 44.1 kHz")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if args.resample:
        torch.set_num_threads(1)
        return resample_leg(args, dev)
    torch.set_num_threads(1)
    pool = ThreadPoolExecutor(16)
    dtype = torch.bfloat16
    head = {"tool": "tools/audioprep_bench.py", "date": datetime.date.today().isoformat(), "commit": args.commit,
            "device": torch.cuda.get_device_name(dev), "out_dtype": "bf16", "max_len": MAX_LEN, "min_len": MIN_LEN}
    print(json.dumps(head), flush=True)
    rows = [head]
    for seconds in (1, 5, 15, 60):
        for fmt in ("int16", "fp32"):
            for B in (int(b) for b in args.batches.split(",")):
                arrs = clips(seconds, fmt, B, seed=B)
                waves = [torch.from_numpy(a.astype(np.float32) / 32768.0 if a.dtype == np.int16 else a) for a in arrs]
                reps = 3 if seconds == 60 and B == 64 else 5

                def collate(feats):
                    wavs = torch.zeros(len(feats), max(w.numel() for w in feats))
                    for i, w in enumerate(feats):
                        wavs[i, : w.numel()] = w
                    return wavs

                def host_1t():
                    return collate([audioprep.postprocess(w, RATE) for w in waves])

                def host_16t():
                    return collate(list(pool.map(lambda w: audioprep.postprocess(w, RATE), waves)))
                host = host_1t()
                h2d_fp32 = device_ms(lambda: host.to(dev), reps=10)
                pack_ms = median_ms(lambda: audioprep.pack_clips(arrs, MAX_LEN, MIN_LEN), reps)
                packed = audioprep.pack_clips(arrs, MAX_LEN, MIN_LEN)
                buf = torch.empty(packed.host.numel(), dtype=torch.uint8, device=dev)
                h2d = device_ms(lambda: buf.copy_(packed.host, non_blocking=True), reps=10)
                ws = torch.empty(max(packed.workspace_bytes, 16), dtype=torch.uint8, device=dev)
                T = packed.T
                out = torch.empty(B, T, dtype=dtype, device=dev)
                base = buf.data_ptr()

                def kernel():
                    hip._check(hip.lib().op_audio_normalize_pad(
                        ctypes.c_void_p(base), packed.src_bytes, ctypes.c_void_p(base + packed.desc_off),
                        packed.desc.ctypes.data_as(ctypes.c_void_p), B, MAX_LEN, MIN_LEN, hip.ptr(out), T, hip.DT_BF16, hip.ptr(ws),
                        ws.numel(), hip.stream()), "op_audio_normalize_pad")
                kernel_ms = device_ms(kernel, reps=20)
                worst = check(out.cpu(), arrs, dtype)
                per = arrs[0].dtype.itemsize
                moved = sum(a.shape[0] * per + min(a.shape[0], MAX_LEN) * per for a in arrs) + out.numel() * out.element_size()
                half = torch.empty(max(moved // 2, 16), dtype=torch.uint8, device=dev)
                dst = torch.empty_like(half)
                copy_ms = device_ms(lambda: dst.copy_(half), reps=20)
                row = {"seconds": seconds, "src": fmt, "B": B, "T": T, "moved_mb": round(moved / 2 ** 20, 2),
                       "host_1t_ms": round(median_ms(host_1t, reps), 3), "host_16t_ms": round(median_ms(host_16t, reps), 3),
                       "h2d_fp32_ms": round(h2d_fp32, 4), "pack_ms": round(pack_ms, 3), "h2d_ms": round(h2d, 4),
                       "kernel_ms": round(kernel_ms, 4), "kernel_gbps": round(moved / kernel_ms / 1e6, 1),
                       "copy_gbps": round(2 * half.numel() / copy_ms / 1e6, 1), "worst_err_over_bound": round(worst, 3)}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del buf, ws, out, packed, half, dst, host
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
