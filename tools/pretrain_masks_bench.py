"""The mask tensors of a pretraining batch: pretrain_masks.ImageTextPretrainMasks / AudioTextPretrainMasks on the device against the same
rules run per sample on one host thread.

    python tools/pretrain_masks_bench.py [--batch 128] [--legs 5] [--reps 20] [--out profiles/pretrain_masks_mi355x.json]

Shapes of pretrain_vl_3B / pretrain_al_3B: 256 patches, captions of up to 70 tokens (+ eos), 15 s of audio = 749 frames.
Rows:
  image_text / audio_text          one call of the generator: the key draw, the launches (three / four), and for width=None the one
                                   device-to-host read of the text id widths; `_bounded`: the same with width = L + 1 (no read)
  op_mask_patches / _words / _blocks   the launch of one mask family alone through ops, on keys drawn before
  each generator row beside `host_ms_one_thread`: the same rules per sample in torch on one host thread (randperm, argsort and
  multinomial per sample, as a dataset's __getitem__ does them), padded into a batch and copied to the device.  That host statement is
  the comparison, not the code under test.
Device times: `legs` legs of `reps` calls timed by the host clock around a device synchronise (the calls are launch-bound, so the
enqueue is what there is to measure), medians over the legs with their spread.  There is no speed gate.  Before timing, the device
result is compared with the CPU route of ops on the same keys, bit for bit."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from one_peace_amd import hip, ops  # noqa: E402
from one_peace_amd.pretrain_masks import AudioTextPretrainMasks, ImageTextPretrainMasks  # noqa: E402


def measure(fn, legs, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(legs):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3 / reps)
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "max_ms": float(max(ms))}


def host_median_ms(fn, runs=5):
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


# ---- the host statement: one sample at a time, torch's own random functions ------------------------------------------------------------
def host_words(tokens, table, p, vl_ratio=None):
    ws = table[tokens].bool()
    starts = ws.nonzero().flatten()
    k = int(math.ceil(ws.float().sum() * p))
    chosen = starts[torch.randperm(starts.numel())[:k]]
    wid = ws.long().cumsum(0)
    m = torch.isin(wid, wid[chosen]) & (wid > 0)
    out = [torch.cat([torch.zeros(1, dtype=torch.bool), m, torch.zeros(1, dtype=torch.bool)])]
    if vl_ratio is not None:
        score = torch.rand(m.numel())
        score[m] = -1.0
        vl = torch.zeros_like(m)
        vl[score.argsort(descending=True)[:int(m.numel() * vl_ratio)]] = True
        out.append(torch.cat([torch.zeros(1, dtype=torch.bool), vl, torch.zeros(1, dtype=torch.bool)]))
    return out


def host_patches(N, m1, extra):
    m = torch.zeros(N, dtype=torch.bool)
    m[torch.randperm(N)[:m1]] = True
    vl = ~m
    masked = m.nonzero().flatten()
    vl[masked[torch.randperm(masked.numel())[:extra]]] = True
    cls = torch.zeros(1, dtype=torch.bool)
    return [torch.cat([cls, m]), torch.cat([cls, vl])]


def host_blocks(T, p, length, adjust):
    K, target = ops.block_counts(T, p, length, adjust)
    m = torch.zeros(T)
    c = torch.randint(0, T, (K,))
    span = (c.view(-1, 1) + torch.arange(length) - length // 2).clamp(0, T - 1)
    m[span.flatten()] = 1
    n = int(m.sum())
    if n > target:
        m[torch.multinomial(m, n - target)] = 0
    elif n < target:
        m[torch.multinomial(1 - m, target - n)] = 1
    return torch.cat([torch.zeros(1, dtype=torch.bool), m.bool()])


def collate(masks, dev):
    mask = torch.nn.utils.rnn.pad_sequence(masks, batch_first=True, padding_value=False)
    ids = torch.nn.utils.rnn.pad_sequence([(~m).nonzero().flatten() for m in masks], batch_first=True, padding_value=-1)
    return mask.to(dev), ids.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--legs", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pretrain_masks_bench: needs a GPU (nothing is measured without one)")
    hip.lib()
    torch.set_num_threads(1)
    B, L, N, T = a.batch, 71, 256, 749
    dev = torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(0)
    vocab = 50265
    table = (torch.rand(vocab, generator=g) < 0.6).to(torch.uint8)   # about 1.7 tokens per word
    table[:4] = 1
    lens = torch.randint(8, 71, (B,), generator=g).tolist()
    tok = torch.full((B, L), 1, dtype=torch.int64)
    for b, n in enumerate(lens):
        tok[b, :n] = torch.randint(4, vocab, (n,), generator=g)
        tok[b, n] = 2
    frames = [T - 37 * (b % 5) for b in range(B)]
    pad = torch.arange(T + 1).expand(B, T + 1) > torch.tensor(frames).view(B, 1)
    vl, al = ImageTextPretrainMasks(table), AudioTextPretrainMasks(table)
    net_vl = {"src_tokens": tok.to(dev)}
    net_al = {"src_tokens": tok.to(dev), "audio_padding_masks": pad.to(dev)}
    dg = torch.Generator(device=dev).manual_seed(0)

    # ---- the device results equal the CPU route's on the same keys ----
    keys = vl.draw_keys(B, L, dev, dg)
    got, want = vl.apply(net_vl, keys), vl.apply({"src_tokens": tok}, {k: v.cpu() for k, v in keys.items()})
    assert all(torch.equal(got[k].cpu(), want[k]) for k in want), "image-text masks: device != host route"
    akeys = al.draw_keys(B, L, frames, T, dev, dg)
    got, want = al.apply(net_al, akeys, frames), al.apply({"src_tokens": tok}, {k: v.cpu() for k, v in akeys.items()}, frames)
    assert all(torch.equal(got[k].cpu(), want[k]) for k in want if k != "audio_padding_masks"), "audio-text masks: device != host route"

    rows = []

    def add(row, fn, host_fn=None):
        row.update({"B": B})
        row.update(measure(fn, a.legs, a.reps))
        if host_fn is not None:
            row["host_ms_one_thread"] = host_median_ms(host_fn)
            row["host_over_device"] = row["host_ms_one_thread"] / row["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)

    def host_vl():
        per = [host_words(tok[b, :lens[b]], table, vl.text_mask_ratio, vl.vl_text_mask_ratio) + host_patches(N, vl.mask_patches, vl.vl_extra)
               for b in range(B)]
        return [collate([s[i] for s in per], dev) for i in range(4)]

    def host_al():
        per = [host_words(tok[b, :lens[b]], table, al.al_text_mask_ratio) + [host_blocks(frames[b], p, al.audio_mask_length, al.audio_mask_prob_adjust)
                                                                           for p in (al.audio_mask_ratio, al.al_audio_mask_ratio)]
               for b in range(B)]
        return [collate([s[i] for s in per], dev) for i in range(3)]

    shapes = {"patches": N, "tokens": L - 1, "frames": T}
    add(dict(case="image_text", tensors=8, launches=3, **shapes), lambda: vl(net_vl, generator=dg), host_vl)
    add(dict(case="image_text_bounded", tensors=8, launches=3, **shapes), lambda: vl(net_vl, generator=dg, width=L + 1))
    add(dict(case="audio_text", tensors=6, launches=4, **shapes), lambda: al(net_al, frames=frames, generator=dg), host_al)
    add(dict(case="audio_text_bounded", tensors=6, launches=4, **shapes), lambda: al(net_al, frames=frames, generator=dg, width=L + 1))
    add(dict(case="audio_text_frames_from_padding_mask", tensors=6, launches=4, **shapes), lambda: al(net_al, generator=dg, width=L + 1))
    add(dict(case="op_mask_patches", **shapes), lambda: ops.patch_masks(keys["image_a"], keys["image_b"], vl.mask_patches, vl.vl_extra))
    dtab = table.to(dev)
    add(dict(case="op_mask_words_vl_bounded", **shapes),
        lambda: ops.word_masks(net_vl["src_tokens"], dtab, keys["text_a"], 0.15, keys["text_b"], 0.4, width=L + 1))
    add(dict(case="op_mask_blocks", **shapes),
        lambda: ops.block_masks(frames, akeys["audio_centers"], akeys["audio_keys"], al.audio_mask_ratio, al.audio_mask_length,
                                al.audio_mask_prob_adjust))

    result = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "legs": a.legs, "reps_per_leg": a.reps,
              "timing": "host clock around `reps` calls and one device synchronise", "rows": rows}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
