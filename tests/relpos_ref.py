"""Shared by tests/test_relpos_ref_cpu.py and tests/test_relpos_fp64_gpu.py: the relative-position bias path -- op_relpos_bias_build,
op_relpos_bias_build_ids, op_relpos_bias_fold_ids, op_relpos_bias_bwd of csrc/elementwise.hip and the pair lists of hip.relpos_pairs --
as exact references, an fp32 re-statement of op_relpos_bias_bwd in the order include/onepeace_hip.h documents (with its mutants), a
checker for the pair lists, the derived budget, the data families and the case lists.  Nothing here needs a GPU.

The operation is a gather (forward) and a scatter-sum (backward), so the gates are sharper than a tolerance:

  forward          bit equality with table[bucket[..]]; pad columns exactly +0.
  `int` family     gradients drawn from {-8 .. 8}: every fp32 partial sum is an integer below 2^24 (at most 1025^2 positions of magnitude
                   8 = 8.4e6 in one bucket; a fold adds a few dozen values per address before that), so fp32 is EXACT in any order and
                   must equal the fp64 sum.  One dropped, doubled or misplaced non-zero position changes an integer: it cannot hide.
  `real` family    randn.  op_relpos_bias_bwd adds in a fixed order with additions only (nothing to contract), so the host emulation
                   below must give the SAME BITS as the kernels.  The budget is only the order-independent backstop.

THE BUDGET (u = 2^-24, gamma(n) = n u / (1 - n u); derived from the operation counts, not fitted)
  table gradient   bucket r with m_r segments: a term passes at most PAIR_SEG additions in pass 1 and m_r in pass 2:
                       E_r = gamma(PAIR_SEG + m_r) sum|x|_r
  fold             an address with c contributions (fp32 atomics, any order): gamma(c - 1) sum|x|; c = 1 is a copy (bit-exact: 0 + x),
                   c = 0 stays +0.
  fold, then table gradient:  gamma(c_max + PAIR_SEG + m_r) sum|x|_r.

TABLE VALUES.  Entry (r, h) holds bf16 pattern number (r heads + h) * 40503 mod P of the P = 65011 first finite normal patterns (both
signs; P prime, so the map is a bijection of 0 .. P-1): all entries are distinct while num_rel * heads <= P; past that (only 3972 x 24)
two entries coincide only if their numbers differ by exactly P, so a neighbouring row, any other head of the same row and any row of the
same head still differ.  A gather from the wrong row or head cannot return the right number.

NOT COVERED: relpos_seg_fold_kernel past the ew_grid cap of 2048 x 256 threads would need num_rel * heads > 524 288; the largest
configuration (the joint table of a 1025-token image, 24 heads) has about 10^5.  The other four grid-stride loops are reached:
build (S Spad), build_ids (B K Kpad), fold_ids (B heads K^2) and seg_sum (nseg heads) -- see `trips`."""
import math

import numpy as np
import torch

from oracle import onepeace_oracle as O
from tests.gemm_ref import SENTINEL, cdiv, check_guard, guarded, guarded_from  # noqa: F401
from tests.rows_ref import guarded_ld, to64  # noqa: F401

BF, F32, I32 = torch.bfloat16, torch.float32, torch.int32
U = 2.0 ** -24
PAIR_SEG = 32      # MIRROR of hip.PAIR_SEG (tests/test_relpos_ref_cpu.py asserts that they agree)
HEADS = (1, 3, 24)
NAN = float("nan")


def gamma(n):
    """n u / (1 - n u) of an fp64 tensor of operation counts."""
    return n * U / (1.0 - n * U)


def attn_spad(S):      # MIRROR of hip.attn_spad
    return cdiv(S, 128) * 128


def ew_grid(items):    # MIRROR of ew_grid in csrc/elementwise.hip
    return max(1, min(2048, cdiv(items, 256)))


def trips(items):
    """Trips of a grid-stride loop over `items` work items: more than one = the launch exceeds the grid cap."""
    return cdiv(items, 256 * ew_grid(items))


def spads(S):
    """The Spad values of a build case: attn_spad(S), S rounded up to 8 and, where it is a multiple of 8, S itself (= the former)."""
    return sorted({attn_spad(S), cdiv(S, 8) * 8})


# ----------------------------------------------------------------------------------------------------------------------
# bucket cases
# ----------------------------------------------------------------------------------------------------------------------
class BucketCase:
    """bucket: int32 [S, S] (possibly an uncopied view of a larger table: stride(0) is the bucket_ld of the launch)."""

    def __init__(self, name, bucket, num_rel):
        self.name, self.bucket, self.S, self.num_rel = name, bucket, bucket.shape[0], num_rel
        assert bucket.dtype == I32 and bucket.shape[0] == bucket.shape[1]
        assert 0 <= int(bucket.min()) and int(bucket.max()) < num_rel      # (index ranges are the caller's contract: no case breaks it)

    @property
    def ld(self):
        return self.bucket.stride(0)


_CACHE = {}


def _image(n):
    num = (2 * n - 1) ** 2 + 3
    return O.image_bucket_position(n, num).to(I32), num


def _token_table():
    if "token" not in _CACHE:
        _CACHE["token"] = O.token_bucket_position(256).to(I32)      # [1024, 1024], CLS buckets added: 2 * 256 - 1 + 3 rows
    return _CACHE["token"], 2 * 256 - 1 + 3


def _joint():
    """relpos.joint_handle's layout (that of test_relpos_table_gradient_over_many_segments): the 257-token image block, a 64-token block
    with its own rows, every other position -> the zero row: one bucket of 321^2 - 257^2 - 64^2 = 32 896 positions."""
    img, num_img = _image(16)
    T = 64
    tb = (torch.arange(T)[None, :] - torch.arange(T)[:, None]).clamp(-31, 31) + 31
    S = img.shape[0] + T
    jb = torch.full((S, S), num_img + 63, dtype=I32)
    jb[:257, :257] = img
    jb[257:, 257:] = tb.to(I32) + num_img
    return jb, num_img + 64


SYNTH_COUNTS = (0, 1, 31, 32, 33, 64, 65, 0, 0, 96, 1)      # then one bucket with the rest of the 24 x 24 positions


def _synthetic():
    S = 24
    counts = list(SYNTH_COUNTS) + [S * S - sum(SYNTH_COUNTS)]
    vals = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts))
    perm = torch.randperm(S * S, generator=torch.Generator().manual_seed(77))
    return vals[perm].view(S, S).to(I32), len(counts)


def _one_each():
    """S = 4, num_rel = 16, one position per bucket: the bound S^2 // PAIR_SEG + num_rel on nseg is the real segment count."""
    return torch.randperm(16, generator=torch.Generator().manual_seed(78)).view(4, 4).to(I32), 16


TOKEN_S = (2, 33, 64, 70, 257)


def bucket_case(name):
    if name not in _CACHE:
        if name.startswith("image"):
            b, num = _image(int(name[5:]))
        elif name.startswith("token"):      # token<S>v: the [:S, :S] view left uncopied (bucket_ld = 1024); token<S>c: a contiguous copy
            tab, num = _token_table()
            S = int(name[5:-1])
            b = tab[:S, :S] if name.endswith("v") else tab[:S, :S].contiguous()
        else:
            b, num = {"joint": _joint, "synthetic": _synthetic, "one_each": _one_each}[name]()
        _CACHE[name] = BucketCase(name, b, num)
    return _CACHE[name]


BUCKET_NAMES = ["image4", "image16", "image32"] + ["token%d%s" % (S, k) for S in TOKEN_S for k in "vc"] + ["joint", "synthetic", "one_each"]
MUTANT_CASES = ("image16", "joint", "synthetic")


# ----------------------------------------------------------------------------------------------------------------------
# data
# ----------------------------------------------------------------------------------------------------------------------
_P = 65011      # the largest prime below 2 * 254 * 128 = 65024 finite normal bf16 patterns
assert all(_P % d for d in range(2, int(math.isqrt(_P)) + 1))


def make_table(num_rel, heads):
    """bf16 [num_rel, heads] (see TABLE VALUES)."""
    n = torch.arange(num_rel * heads, dtype=torch.int64)
    k = (n * 40503) % _P
    pat = (k >> 1) + 0x0080 + (k & 1) * 0x8000      # magnitude patterns 0x0080 .. 0x7F7F: normal, finite
    pat = torch.where(pat >= 0x8000, pat - 0x10000, pat).to(torch.int16)
    return pat.view(BF).view(num_rel, heads)


def make_grad(family, shape, live, seed):
    """fp32 gradient of `shape` [..., rows, cols]: columns >= live hold NaN (the kernels must not read them).  int: {-8 .. 8}; real: randn."""
    g = torch.Generator().manual_seed(52000 + seed)
    if family == "int":
        x = torch.randint(-8, 9, shape, generator=g).float()
    else:
        x = torch.randn(shape, generator=g)
    x[..., live:] = NAN
    return x


ID_KINDS = ("sorted", "unsorted", "repeats", "mixed", "shared0")


def make_ids(kind, B, K, Sfull, seed=0):
    """int32 [B, K] position ids in [0, Sfull).
    sorted    CLS (0) first, then a sorted sample of the other positions: what the adapters make.
    unsorted  a random sample in random order.
    repeats   `sorted`, then every fifth slot and the last two take the id of another slot (padding mapped to a valid id).
    mixed     sample b is sorted / unsorted / with repeats / the identity (ids[b, i] = i) for b % 4 = 0 / 1 / 2 / 3.
    shared0   `unsorted`, but every sample holds id 0 at slot 0 and at two more slots and nowhere else: 9 B additions onto
              dense[h][0][0], the contention case of the fold's atomics (needs K >= 3)."""
    g = torch.Generator().manual_seed(53000 + seed)

    def srt():
        return torch.cat([torch.zeros(1, dtype=torch.int64), 1 + torch.randperm(Sfull - 1, generator=g)[:K - 1].sort().values]) if K > 1 else torch.zeros(1, dtype=torch.int64)

    def uns():
        return torch.randperm(Sfull, generator=g)[:K]

    def rep():
        r = srt()
        for s in list(range(4, K, 5)) + [K - 2, K - 1]:
            if s > 0:
                r[s] = r[int(torch.randint(0, max(s, 1), (1,), generator=g))]
        return r

    rows = []
    for b in range(B):
        if kind == "mixed":
            rows.append([srt, uns, rep, lambda: torch.arange(K)][b % 4]())
        elif kind == "shared0":
            assert K >= 3
            r = 1 + torch.randperm(Sfull - 1, generator=g)[:K]
            r[0] = 0
            r[1 + torch.randperm(K - 1, generator=g)[:2]] = 0
            rows.append(r)
        else:
            rows.append({"sorted": srt, "unsorted": uns, "repeats": rep}[kind]())
    ids = torch.stack(rows).to(I32)
    assert ids.shape == (B, K) and int(ids.min()) >= 0 and int(ids.max()) < Sfull
    return ids


# (B, K, Kpad, bucket case of the full positions, heads, id kinds)
IDS_CASES = [
    (5, 9, 128, "image4", 3, ID_KINDS),
    (3, 64, 64, "image16", 3, ID_KINDS),                       # no pad columns
    (4, 120, 128, "image16", 24, ID_KINDS),
    (5, 300, 384, "image32", 2, ("mixed", "shared0")),         # B K Kpad = 576 000 and B heads K^2 = 900 000 > 2048 * 256
    (1, 1, 8, "image4", 3, ("sorted", "unsorted")),
]


# ----------------------------------------------------------------------------------------------------------------------
# references (torch, on the device of their inputs)
# ----------------------------------------------------------------------------------------------------------------------
def image_ref(table, bucket, Spad, transposed=False):
    """bf16 [heads, S, Spad]: table[bucket[i, j], h] at [h, i, j] (transposed: at [h, j, i]); columns >= S are +0."""
    S, heads = bucket.shape[0], table.shape[1]
    v = table[bucket.long()].permute(2, 0, 1)
    out = torch.zeros(heads, S, Spad, dtype=table.dtype, device=table.device)
    out[:, :, :S] = v.transpose(1, 2) if transposed else v
    return out


def image_ids_ref(table, bucket, ids, Kpad, transposed=False):
    """bf16 [B, heads, K, Kpad]: table[bucket[ids[b, i], ids[b, j]], h]."""
    B, K = ids.shape
    i = ids.long()
    v = table[bucket.long()[i[:, :, None], i[:, None, :]]].permute(0, 3, 1, 2)
    out = torch.zeros(B, table.shape[1], K, Kpad, dtype=table.dtype, device=table.device)
    out[..., :K] = v.transpose(2, 3) if transposed else v
    return out


def fold_ref(dbias, ids, Sfull):
    """The fp64 scatter of dbias[b, h, i, j] (j < K) onto dense[h, ids[b, i], ids[b, j]] -> (dense [heads, Sfull, Sfull] fp64, sum|x| per
    address, contributions per address [Sfull, Sfull])."""
    B, heads, K, _ = dbias.shape
    i = ids.long()
    addr = (i[:, :, None] * Sfull + i[:, None, :]).reshape(-1)
    x = dbias[..., :K].double().permute(1, 0, 2, 3).reshape(heads, -1)
    z = torch.zeros(heads, Sfull * Sfull, dtype=torch.float64, device=dbias.device)
    dense = z.clone().index_add_(1, addr, x)
    absum = z.index_add_(1, addr, x.abs())
    count = torch.bincount(addr, minlength=Sfull * Sfull)
    return dense.view(heads, Sfull, Sfull), absum.view(heads, Sfull, Sfull), count.view(Sfull, Sfull)


_LANES = 64


def dtable_ref(dbias, bucket, num_rel):
    """fp64 index_add_ of dbias[:, :, :S] by bucket -> (dtable [num_rel, heads] fp64, sum|x| per bucket and head, positions per bucket)."""
    S, heads = bucket.shape[0], dbias.shape[0]
    b = bucket.reshape(-1).long()
    x = dbias[:, :, :S].double().reshape(heads, -1).t()
    # position p adds into slot p % LANES of its bucket and the slots are summed afterwards: on a device index_add_ adds with atomics, and
    # the 32 896 positions of the joint case's zero-row bucket on ONE address took seconds.  (fp64 either way; exact for the `int` family.)
    lanes = b * _LANES + torch.arange(b.numel(), device=b.device) % _LANES
    z = torch.zeros(num_rel * _LANES, heads, dtype=torch.float64, device=dbias.device)
    tot, absum = (z.clone().index_add_(0, lanes, v).view(num_rel, _LANES, heads).sum(1) for v in (x, x.abs()))
    return tot, absum, torch.bincount(b, minlength=num_rel)


def bwd_budget(absum, counts, extra=0):
    """E_r = gamma(PAIR_SEG + m_r + extra) sum|x|_r, [num_rel, heads]."""
    m = (counts.double() + PAIR_SEG - 1).div(PAIR_SEG).floor()
    return gamma(PAIR_SEG + m + extra)[:, None] * absum


def fold_budget(absum, count):
    return gamma((count.double() - 1).clamp_min(0))[None] * absum


# ----------------------------------------------------------------------------------------------------------------------
# the pair lists
# ----------------------------------------------------------------------------------------------------------------------
def np_lists(lists):
    pos, seg, bucket_seg, nseg = lists
    return pos.cpu().numpy().astype(np.int64), seg.cpu().numpy().astype(np.int64), bucket_seg.cpu().numpy().astype(np.int64), int(nseg)


def check_pairs(lists, bucket, num_rel):
    """The failures of (pos, seg, bucket_seg, nseg) as the pair lists of bucket [S, S] ([] = sound)."""
    pos, seg, bs, nseg = np_lists(lists)
    S = bucket.shape[0]
    b = bucket.cpu().numpy().astype(np.int64).reshape(-1)
    f = []
    if len(seg) != nseg + 1:
        return ["len(seg) = %d, nseg + 1 = %d" % (len(seg), nseg + 1)]
    if len(bs) != num_rel + 1 or len(pos) != S * S:
        return ["len(bucket_seg) = %d, len(pos) = %d" % (len(bs), len(pos))]
    if not np.array_equal(np.sort(pos), np.arange(S * S)):
        f.append("pos is no permutation of 0 .. S^2 - 1")
        return f
    if bs[0] != 0 or np.any(np.diff(bs) < 0):
        f.append("bucket_seg is not monotone from 0")
    real = int(bs[num_rel])
    if real > nseg:
        return f + ["%d real segments, nseg = %d" % (real, nseg)]
    if np.any(seg[real:] != S * S):
        f.append("a segment past the real ones is not empty")
    if real and seg[0] != 0:
        f.append("the first segment does not start at 0")
    ln = np.diff(seg)
    if np.any(ln < 0) or np.any(ln[:real] < 1) or np.any(ln > PAIR_SEG):
        f.append("segment lengths outside 1 .. PAIR_SEG (real) or negative")
        return f
    counts = np.bincount(b, minlength=num_rel)
    if not np.array_equal(np.diff(bs), (counts + PAIR_SEG - 1) // PAIR_SEG):
        f.append("bucket r does not own ceil(count_r / PAIR_SEG) segments")
        return f
    seg_bucket = np.repeat(np.arange(num_rel), np.diff(bs))              # bucket of every real segment
    k_seg = np.repeat(np.arange(real), ln[:real])                        # segment of every list slot
    if len(k_seg) != S * S:
        return f + ["the real segments cover %d of %d positions" % (len(k_seg), S * S)]
    if not np.array_equal(b[pos], seg_bucket[k_seg]):
        f.append("a segment holds a position of another bucket")
    same = b[pos][1:] == b[pos][:-1]
    if np.any(np.diff(pos)[same] <= 0):
        f.append("positions do not ascend inside a bucket")
    return f


# ----------------------------------------------------------------------------------------------------------------------
# op_relpos_bias_bwd in NumPy fp32, in the documented order
# ----------------------------------------------------------------------------------------------------------------------
BWD_MUTANTS = ("dropped", "twice", "swap_ij", "head_stride", "seg_boundary", "pad_column", "bucket_seg_shift")


def emulate_bwd(dbias, S, Spad, lists, num_rel, mutant=None):
    """fp32 [num_rel, heads] with the bits op_relpos_bias_bwd must return.  Pass 1: per segment and head, s = 0, then + every position of
    pos[seg[t] .. seg[t+1]) in order; pass 2: per bucket, s = 0, then + every segment's sum in order.  Vectorised over segments / buckets.
    The mutants pick a position whose head-0 value is non-zero, so that the `int` family shows them too; pad_column needs Spad > S."""
    pos, seg, bs, nseg = np_lists(lists)
    d = np.ascontiguousarray(dbias.cpu().numpy(), dtype=np.float32)
    heads = d.shape[0]
    flat = d.reshape(-1)
    hoff = (np.arange(heads, dtype=np.int64) * (S * S if mutant == "head_stride" else S * Spad))[:, None]
    zero = np.float32(0)

    def offs(p):
        i = p // S
        j = p - i * S
        return (j * Spad + i) if mutant == "swap_ij" else (i * Spad + j)

    hit = None
    if mutant in ("dropped", "twice", "pad_column"):      # (segment, step): in the first segment of the largest bucket
        r = int(np.argmax(np.diff(bs)))
        t0 = int(bs[r])
        nz = np.nonzero(flat[offs(pos[seg[t0]:seg[t0 + 1]])])[0]
        hit = (t0, int(nz[0]))
    elif mutant == "seg_boundary":      # the first position of a bucket is handed to the last segment of the bucket before it
        first = bs[:-1][np.diff(bs) > 0][1:]
        first = [t for t in first if flat[offs(pos[seg[t]])] != 0]
        seg = seg.copy()
        seg[first[len(first) // 2]] += 1
    elif mutant == "bucket_seg_shift":
        bs = np.minimum(bs + 1, nseg)
    lo, hi = seg[:-1], seg[1:]
    partial = np.zeros((heads, nseg), dtype=np.float32)
    for k in range(int((hi - lo).max())):
        idx = lo + k
        valid = idx < hi
        off = offs(pos[np.minimum(idx, S * S - 1)])
        if hit is not None and hit[1] == k:
            if mutant == "dropped":
                valid = valid.copy()
                valid[hit[0]] = False
            elif mutant == "pad_column":
                off[hit[0]] = off[hit[0]] // Spad * Spad + S
        v = np.where(valid[None, :], flat[hoff + off[None, :]], zero)
        partial += v
        if hit is not None and hit[1] == k and mutant == "twice":
            partial[:, hit[0]] += v[:, hit[0]]
    lo, hi = bs[:-1], bs[1:]
    dt = np.zeros((heads, num_rel), dtype=np.float32)
    for k in range(int((hi - lo).max())):
        t = lo + k
        dt += np.where((t < hi)[None, :], partial[:, np.minimum(t, nseg - 1)], zero)
    return torch.from_numpy(np.ascontiguousarray(dt.T))


def share(got, exact, E):
    """(largest |got - exact| / E over the elements with E > 0, number of elements with E == 0 that differ)."""
    err = (got.double() - exact).abs()
    pos = E > 0
    s = float((err[pos] / E[pos]).max()) if bool(pos.any()) else 0.0
    return s, int((err[~pos] != 0).sum())
