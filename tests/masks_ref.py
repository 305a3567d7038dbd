"""Loop-level restatement of the pretraining-mask rules (one sample at a time, Python lists and ints), written from the rules alone:
it shares no code with one_peace_amd.ops.  Every function returns plain lists; pack() pads them to collate_fn's layout."""
import math

import numpy as np
import torch


def select(cand, k, keys):
    """The k items first in the order (key descending, index ascending) over the candidates; the other items follow in index order."""
    order = sorted((i for i in range(len(cand)) if cand[i]), key=lambda i: (-int(keys[i]), i))
    order += [i for i in range(len(cand)) if not cand[i]]
    assert 0 <= k <= len(order), (k, len(order))
    return order[:k]


def preserve(mask):
    return [i for i, m in enumerate(mask) if not m]


def patches(keys_a, keys_b, m1, extra):
    """-> (image mask with CLS, vl mask with CLS) of one image; keys: N ints each."""
    N = len(keys_a)
    m = [False] * N
    for i in select([True] * N, m1, keys_a):
        m[i] = True
    vl = [not x for x in m]
    for i in select(m, extra, keys_b):
        vl[i] = True
    return [False] + m, [False] + vl


def words_k(W, p):
    """ceil of the float32 product float32(W) * float32(p)."""
    return int(math.ceil(np.float32(W) * np.float32(p)))


def words(row, table, keys_a, p, keys_b=None, vl_ratio=None, pad=1):
    """row: the L token ids of one sample (tokens, eos, pads).  -> (mask, vl mask or None), each of the row's OWN length nonpad + 1
    (CLS, tokens, eos), and n."""
    nonpad = sum(1 for t in row if t != pad)
    n = max(nonpad - 1, 0)
    ws = [0 <= row[t] < len(table) and table[row[t]] != 0 for t in range(n)]
    W = sum(ws)
    k = words_k(W, p) if n and W else 0
    m = [False] * n
    for s in select(ws, k, keys_a[:n]):
        m[s] = True
        u = s + 1
        while u < n and not ws[u]:
            m[u] = True
            u += 1
    tail = [False] * (nonpad - n)  # eos
    vl = None
    if keys_b is not None:
        k2 = int(n * vl_ratio)
        vl = [False] * n
        for i in select([not x for x in m], k2, keys_b[:n]):
            vl[i] = True
        vl = [False] + vl + tail
    return [False] + m + tail, vl, n


def block_counts(T, p, length, adjust):
    return int(T * ((p + adjust) / length)), int(T * p)


def blocks(T, centers, keys, p, length, adjust):
    """-> (mask with CLS, of length T + 1; the case: 'over', 'under' or 'equal')."""
    K, target = block_counts(T, p, length, adjust)
    m = [False] * T
    for c in list(centers)[:K]:
        for i in range(length):
            m[min(max(int(c) + i - length // 2, 0), T - 1)] = True
    n = sum(m)
    case = "over" if n > target else ("under" if n < target else "equal")
    if n > target:
        for i in select(m, n - target, keys[:T]):
            m[i] = False
    elif n < target:
        for i in select([not x for x in m], target - n, keys[:T]):
            m[i] = True
    assert sum(m) == target
    return [False] + m, case


def pack(masks, S, width=None):
    """collate_fn's layout of per-sample masks: (bool [B, S] padded with False, int64 [B, width] of the kept positions padded with -1;
    width=None: the batch maximum)."""
    B = len(masks)
    keep = [preserve(m) for m in masks]
    if width is None:
        width = max([len(k) for k in keep] + [0])
    out = torch.zeros(B, S, dtype=torch.bool)
    ids = torch.full((B, width), -1, dtype=torch.int64)
    for b, m in enumerate(masks):
        out[b, :len(m)] = torch.tensor(m, dtype=torch.bool)
        kk = keep[b][:width]
        ids[b, :len(kk)] = torch.tensor(kk, dtype=torch.int64)
    return out, ids
