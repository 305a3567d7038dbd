"""Shared by tests/test_attention_ref_cpu.py and tests/test_attention_fp64_gpu.py: the fp64 attention forward / backward in closed
form, the model of the roundings the HIP kernels document, per-(sample, head) error norms, the gate built from them, mutants of
the model (one per class of subtle kernel bug), and the seeded input families and key-pad patterns.

Layout here: q, k, v, dout [B, heads, S, 64]; bias [heads, S, S] (shared) or [B, heads, S, S] (per sample); key_pad [B, S] bool
(True = masked key) or None.  Every input holds bf16 VALUES (built in bf16, then upcast), so the reference and a kernel see the
same numbers.  Nothing here needs a GPU; everything runs on whatever device its inputs live on, one sample at a time.

A row whose keys are ALL masked has no softmax (NaN here as in the kernels): out of scope, no pattern below produces one."""
import math

import torch

U32 = 2.0 ** -24   # fp32 unit roundoff
HD = 64
SCALE = 0.125
KINDS = ("out", "lse", "dq", "dk", "dv", "dbias")

# The gate, per output kind and per (sample, head) slice:   ||got - exact|| <= MARGINS[kind] * ||model - exact|| + floor.
# MARGINS = 1.5 x MEASURED_MAX_RATIO, the largest ||got - exact|| / ||model - exact|| over all 500 cases of
# tests/test_attention_fp64_gpu.py on the MI355X (profiles/attention_fp64_errors_mi355x.jsonl, one line per case; no case was set
# aside as a finding); the 1.5 covers the order of the fp32 sums, which differs between routes and with the CU count that sets the
# batch chunking.  The medians are 1.00 (out, dv), 1.01 (dq), 1.02 (dk), 0.93 (dbias): the kernels make the model's error and
# little else.  The maxima of dq / dk come from the `offset` family (dk 1.18 ... 1.72 there, 1.13 at most elsewhere): a forward
# kernel rounds exp(s - RUNNING max) tile by tile, the model exp(s - row max); the resulting bf16 `out` differs in single ulps,
# delta with it, and dk = scale * dS^T q multiplies that row-wise difference by the large q component the family shares (a CPU
# emulation of the tile-wise rounding gives 1.37 and 1.74 where the kernels measure 1.37 and 1.72).  lse: the model's only error
# is the fp32 storage rounding, below the floor on every slice, so the floor alone gates it (measured: <= 0.25 of the floor).
# tests/test_attention_ref_cpu.py bounds the margins from above: every mutant below must still fail the gate (the weakest, a
# dropped dS column at peaked scores, needs 3.0 in dq and 3.3 in dk to pass).
MEASURED_MAX_RATIO = {"out": 1.011, "lse": 1.0, "dq": 1.131, "dk": 1.722, "dv": 1.101, "dbias": 1.258}
MARGINS = {k: 1.5 * v for k, v in MEASURED_MAX_RATIO.items()}
# floor = FLOOR_ULPS fp32 ulps of the slice's largest term, as a norm: x sqrt(elements of the slice).  The kernels accumulate in
# fp32: a sum of n terms carries ~sqrt(n) ... n half-ulps of its largest partial sum, a few ulps for the 64 ... 1025-term sums here
# once measured against the sum of the terms' MAGNITUDES (`magnitudes` in _attn: max |v| for out; scale * sum |q| |k| + |bias| +
# log S for lse; |dout| x the largest column sum of P for dv; for dq / dk / dbias the cancellation-free bound
# P * (sum |dout| |v| + sum |dout| |out|) on |dS|, summed along the contracted axis, times scale * max |k| resp. max |q|).  It
# decides alone where the model's own error vanishes: one valid key has P = 1 exactly, out = v, dS = 0 (measured there and on
# every other slice below the floor: <= 0.15 of the floor for out, 0.25 lse, 0.04 dq, 1.19 dk -- inside margin x model + floor).
FLOOR_ULPS = 4.0


def bf(x):
    """Round to bf16 and back (round-to-nearest-even, as the kernels' conversions)."""
    return x.to(torch.bfloat16).to(x.dtype)


MUTANTS = ("drop_last_key_ds", "attend_first_padded", "skip_rescale", "bias_block_transposed", "delta_neighbour_head",
           "dbias_last_chunk_missing", "lse_without_bias")


def _attn(q, k, v, bias, key_pad, dout, scale, model, mutant=None, per_sample_dbias=False, chunk=2):
    B, heads, S, _ = q.shape
    dev = q.device
    per_sample = bias is not None and bias.dim() == 4
    keep = per_sample or per_sample_dbias
    out, lse_o, dq, dk, dv, dbs = [], [], [], [], [], []
    db_sum = torch.zeros(heads, S, S, dtype=torch.float64, device=dev) if bias is not None and not per_sample else None
    mags = {n: [] for n in ("out", "lse", "dq", "dk", "dv", "dbias")}
    dbmag_sum = torch.zeros_like(db_sum) if db_sum is not None else None
    b0, h0 = B - 1, heads - 1   # the (sample, head) the single-item mutants hit
    nb_f = B - (B % chunk or chunk) if mutant == "dbias_last_chunk_missing" else B   # samples that reach the summed dbias
    for b in range(B):
        qb, kb, vb, dob = (t[b].double() for t in (q, k, v, dout))
        qk = (qb * scale) @ kb.transpose(-1, -2)
        bb = None
        if bias is not None:
            bb = (bias[b] if per_sample else bias).double()
            if mutant == "bias_block_transposed" and b == b0:   # the same 512 values, walked key-major
                bb = bb.clone()
                bb[h0, :16, :32] = bb[h0, :16, :32].t().reshape(16, 32)
        s = qk if bb is None else qk + bb
        pad = key_pad[b].clone() if key_pad is not None else torch.zeros(S, dtype=torch.bool, device=dev)
        if mutant == "attend_first_padded" and b == b0 and bool(pad.any()):
            pad[int(pad.nonzero()[0])] = False
        s = s.masked_fill(pad[None, None, :], float("-inf"))
        m = s.max(-1, keepdim=True).values
        e = torch.exp(s - m)
        l = e.sum(-1, keepdim=True)
        p = e / l
        lse = (m + torch.log(l)).squeeze(-1)
        changed = False
        if mutant == "skip_rescale" and b == b0 and int((~pad).nonzero()[-1]) >= 64:
            # online softmax over 64-key tiles; at the last tile that holds a valid key the accumulators of queries 0..15 of head
            # h0 keep the previous running maximum's scale: every earlier tile weighs exp(m_final - m_prev) too much
            t0 = (int((~pad).nonzero()[-1]) // 64) * 64
            rows = slice(0, min(16, S))
            m_prev = s[h0, rows, :t0].max(-1, keepdim=True).values
            w = torch.exp(s[h0, rows] - m[h0, rows])
            w[:, :t0] = w[:, :t0] * torch.exp(m[h0, rows] - m_prev)
            w = torch.where(torch.isfinite(w), w, torch.zeros_like(w))
            lw = w.sum(-1, keepdim=True)
            p = p.clone()
            lse = lse.clone()
            p[h0, rows] = w / lw
            e, l = e.clone(), l.clone()
            e[h0, rows], l[h0, rows] = w, lw
            lse[h0, rows] = (m[h0, rows] + torch.log(lw)).squeeze(-1)
            changed = True
        if mutant == "lse_without_bias" and b == b0 and bb is not None:
            rows = slice(0, min(16, S))
            lse = lse.clone()
            lse[h0, rows] = torch.logsumexp(qk[h0, rows].masked_fill(pad[None, :], float("-inf")), dim=-1)
            changed = True
        if model:
            lse = lse.float().double()                        # lse is stored in fp32
        if model:
            # P rounded to bf16 before the PV product -- as the forward kernels round it: the softmax NUMERATOR exp(s - max), with
            # the fp32 row sum divided out of the fp32 product afterwards (rounding the normalised P instead is as large an error
            # but another realisation of it: where dS is mostly cancellation -- saturated rows, the `offset` family -- the two
            # differ per slice by factors of 2 ... 7 in dq / dk, which is what a first run of the kernels against that variant
            # showed, to four digits); then out rounded to bf16
            ob = bf((bf(e) @ vb) / l)
        else:
            ob = p @ vb
        # backward: P again from the stored lse (what the kernels do); in exact arithmetic that is p itself
        pb = torch.exp(s - lse[..., None]) if (model or changed) else p
        dp = dob @ vb.transpose(-1, -2)
        delta = (dob * ob).sum(-1, keepdim=True)              # from the bf16 out in the model
        if mutant == "delta_neighbour_head" and b == b0:
            delta = delta.roll(1, 0)
        ds = pb * (dp - delta)
        if model:
            ds = bf(ds)                                       # dS rounded to bf16 before the dQ and dK products
        if mutant == "drop_last_key_ds" and b == b0:
            ds = ds.clone()
            ds[h0, :, int((~pad).nonzero()[-1])] = 0
        dvb = (bf(pb) if model else pb).transpose(-1, -2) @ dob
        dqb = (ds @ kb) * scale
        dkb = (ds.transpose(-1, -2) @ qb) * scale
        if model:
            dqb, dkb, dvb = bf(dqb), bf(dkb), bf(dvb)
        out.append(ob); lse_o.append(lse); dq.append(dqb); dk.append(dkb); dv.append(dvb)
        if bias is not None:
            if keep:
                dbs.append(ds)
            if db_sum is not None and b < nb_f:
                db_sum += ds                                  # summed in high precision from the (bf16) dS
        if not model and mutant is None:
            # magnitudes: the largest term of every output's sum, per head -- what an fp32 ulp is measured against
            valid = ~pad
            dsmag = p * (dob.abs() @ vb.abs().transpose(-1, -2) + (dob.abs() * ob.abs()).sum(-1, keepdim=True))
            sabs = (qb.abs() * scale) @ kb.abs().transpose(-1, -2)
            if bb is not None:
                sabs = sabs + bb.abs()
            sabs = sabs.masked_fill(pad[None, None, :], 0.0)
            mags["out"].append(vb[:, valid].abs().amax((-1, -2)))
            mags["lse"].append(sabs.amax((-1, -2)) + math.log(S))
            mags["dv"].append(dob.abs().amax((-1, -2)) * p.sum(-2).amax(-1))
            mags["dq"].append(scale * kb.abs().amax((-1, -2)) * dsmag.sum(-1).amax(-1))
            mags["dk"].append(scale * qb.abs().amax((-1, -2)) * dsmag.sum(-2).amax(-1))
            if bias is not None:
                if per_sample:
                    mags["dbias"].append(dsmag.amax((-1, -2)))
                else:
                    dbmag_sum += dsmag
    res = {"out": torch.stack(out), "lse": torch.stack(lse_o), "dq": torch.stack(dq), "dk": torch.stack(dk), "dv": torch.stack(dv)}
    if bias is not None:
        res["dbias"] = torch.stack(dbs) if per_sample else db_sum
        if keep:
            res["dbias_per_sample"] = torch.stack(dbs)
    if not model and mutant is None:
        mg = {n: torch.stack(x) for n, x in mags.items() if x}
        if dbmag_sum is not None:
            mg["dbias"] = dbmag_sum.amax((-1, -2))
        res["magnitudes"] = mg
    return res


def attn_exact(q, k, v, bias, key_pad, dout, scale=SCALE, per_sample_dbias=False):
    """Closed-form fp64 attention forward and backward.  Returns out, dq, dk, dv [B, heads, S, 64], lse [B, heads, S], dbias
    ([heads, S, S] summed over the batch for a shared bias, [B, heads, S, S] for a per-sample one; dbias_per_sample on request)
    and `magnitudes`: per slice, the largest term of each output's sum (the floor of the gate is measured in fp32 ulps of it)."""
    return _attn(q, k, v, bias, key_pad, dout, scale, model=False, per_sample_dbias=per_sample_dbias)


def attn_rounding_model(q, k, v, bias, key_pad, dout, scale=SCALE, mutant=None, chunk=2):
    """attn_exact with the roundings the kernels document and no others: P (unnormalised) -> bf16 before P V; out -> bf16; lse in fp32;
    delta from the bf16 out; P of the backward pass recomputed from the stored lse; dS -> bf16 before the dQ / dK products;
    dq, dk, dv -> bf16; dbias summed in high precision from the bf16 dS.  Its distance from attn_exact is the error a correct
    kernel is allowed to make.  mutant: one of MUTANTS (see the module docstring of the CPU test)."""
    assert mutant is None or mutant in MUTANTS, mutant
    return _attn(q, k, v, bias, key_pad, dout, scale, model=True, mutant=mutant, chunk=chunk)


def per_item_error(got, exact, kind):
    """||got - exact|| per (sample, head) slice: [B, heads] for out / dq / dk / dv / lse and a per-sample dbias, [heads] for a
    shared (batch-summed) dbias.  No norm crosses a slice.  Non-finite differences give inf."""
    d = got.double() - exact.double()
    dims = (-1,) if kind == "lse" else (-1, -2)
    n = torch.linalg.vector_norm(d, dim=dims)
    return torch.where(torch.isfinite(n), n, torch.full_like(n, float("inf")))


def slice_elems(exact, kind):
    return exact.shape[-1] if kind == "lse" else exact.shape[-1] * exact.shape[-2]


def gate_floor(ex, kind):
    """FLOOR_ULPS fp32 ulps of the slice's largest term, as a norm over the slice."""
    return FLOOR_ULPS * U32 * ex["magnitudes"][kind] * math.sqrt(slice_elems(ex[kind], kind))


def gate(got, ex, mdl, kinds=None, margins=None):
    """Checks every output kind of `got` (a dict like attn_exact's) on every slice.  Returns (failures, ratios):
    failures: strings naming kind, slice, error and bound; ratios: kind -> largest ||got - exact|| / ||model - exact|| over the
    slices whose model error exceeds the floor (None when there is no such slice)."""
    margins = margins or MARGINS
    failures, ratios = [], {}
    for kind in kinds or [n for n in KINDS if n in got]:
        e = per_item_error(got[kind], ex[kind], kind)
        em = per_item_error(mdl[kind], ex[kind], kind)
        fl = gate_floor(ex, kind)
        bound = margins[kind] * em + fl
        bad = ~(e <= bound)
        if bool(bad.any()):
            idx = bad.nonzero()[0].tolist()
            i = tuple(idx)
            failures.append("%s%s: err %.3e > %.3g x model %.3e + floor %.3e (%d of %d slices)" % (
                kind, idx, float(e[i]), margins[kind], float(em[i]), float(fl[i]), int(bad.sum()), bad.numel()))
        big = em > fl
        ratios[kind] = float((e[big] / em[big]).max()) if bool(big.any()) else None
        if not bool(big.all()):   # slices whose model error is below the floor: the error as a fraction of the floor
            ratios[kind + "_of_floor"] = float((e[~big] / fl[~big].clamp_min(1e-300)).max())
    return failures, ratios


# ----------------------------------------------------------------------------------------------------------------------
# key-pad patterns
# ----------------------------------------------------------------------------------------------------------------------
PADS = ("none", "tail", "hole", "first_tile", "one_valid")
TAILS = (0, 1, 16, 80, 130, 37, 64)   # ragged tails: nothing, one key, a whole 16-key block, whole 64-key tiles and more


def make_pad(name, B, S):
    """[B, S] bool (True = masked) or None; None too where the pattern does not fit the length (S too short)."""
    if name == "none":
        return None
    pad = torch.zeros(B, S, dtype=torch.bool)
    if name == "tail":
        for b in range(B):
            t = min(TAILS[b % len(TAILS)], S - 1)
            pad[b, S - t:] = True
        if not bool(pad.any()):
            pad[B - 1, S - min(1, S - 1):] = S > 1
    elif name == "hole":          # the joint vl stream: 64 text slots of which 40 are used, then the image tokens
        if S < 64:
            return None
        pad[:, 40:64] = True
        pad[0, 40:64] = B == 1    # (sample 0 of a batch has a full-length text)
    elif name == "first_tile":    # a whole leading key tile masked (16-key block for short sequences)
        n = 64 if S > 64 else 16 if S > 16 else 0
        if n == 0:
            return None
        pad[:, :n] = True
    elif name == "one_valid":
        pad[:] = True
        for b in range(B):
            pad[b, (S - 1, 0, S // 2)[b % 3]] = False
    else:
        raise ValueError(name)
    return pad


# ----------------------------------------------------------------------------------------------------------------------
# input families
# ----------------------------------------------------------------------------------------------------------------------
FAMILIES = ("unit", "peaked", "winner_late", "winner_first", "ascending", "offset", "bias_dominant", "edge_pad")


def make_inputs(family, B, heads, S, key_pad=None, per_sample_bias=False, use_bias=True, seed=0):
    """q, k, v, bias, dout as float32 tensors holding bf16 values (CPU, fixed seed).
    unit: standard normal everything (logit std 1).  peaked: q, k x 3 (logit std ~9).
    winner_late / winner_first: every query has one dominant key (+12) among the last / first 16 valid keys.
    ascending: the logits rise by ~2 per 16 keys along a shared direction, so every key tile moves the running maximum.
    offset: +60 on every logit of a row through a shared q . k component (the max subtraction).
    bias_dominant: bias uniform in +-30 over q . k of std 0.1.
    edge_pad: the strongest key (+12) of every row at the last valid position before the first masked one, a stronger one (+18)
    AT the first masked position (without a pad: only the strong last key)."""
    g = torch.Generator().manual_seed(1000 * FAMILIES.index(family) + seed)
    rn = lambda *sh: torch.randn(*sh, generator=g)
    q, k, v, dout = rn(B, heads, S, HD), rn(B, heads, S, HD), rn(B, heads, S, HD), rn(B, heads, S, HD)
    bshape = (B, heads, S, S) if per_sample_bias else (heads, S, S)
    bias = rn(*bshape) if use_bias else None
    u = torch.zeros(HD)
    u[::2] = 1.0 / math.sqrt(HD / 2)   # a unit direction shared by q and k
    valid = ~key_pad if key_pad is not None else torch.ones(B, S, dtype=torch.bool)
    if family == "peaked":
        q, k = 3 * q, 3 * k
    elif family in ("winner_late", "winner_first"):
        for b in range(B):
            idx = valid[b].nonzero().flatten()
            pool = idx[-16:] if family == "winner_late" else idx[:16]
            w = pool[torch.arange(S) % len(pool)]
            kw = k[b][:, w]                                   # [heads, S, 64]: the winner's key per query
            q[b] = q[b] + (12.0 / SCALE) * kw / (kw * kw).sum(-1, keepdim=True)
    elif family == "ascending":
        q = 0.5 * q + 4.0 * u
        k = k + (0.25 * torch.arange(S, dtype=torch.float32))[:, None] * u
    elif family == "offset":
        a = math.sqrt(60.0 / SCALE)
        q, k = q + a * u, k + a * u
    elif family == "bias_dominant":
        q, k = 0.3 * q, 0.3 * k
        if use_bias:
            bias = torch.rand(*bshape, generator=g) * 60 - 30
    elif family == "edge_pad":
        q = q + 3.0 * u
        for b in range(B):
            masked = (~valid[b]).nonzero().flatten()
            fp = int(masked[0]) if len(masked) else -1
            lv = fp - 1 if fp > 0 else int(valid[b].nonzero()[-1])
            k[b, :, lv] += (12.0 / (SCALE * 3.0)) * u
            if fp >= 0:
                k[b, :, fp] += (18.0 / (SCALE * 3.0)) * u
    elif family != "unit":
        raise ValueError(family)
    r = lambda t: None if t is None else t.to(torch.bfloat16).float()
    return r(q), r(k), r(v), r(bias), r(dout)


# ----------------------------------------------------------------------------------------------------------------------
# the kernels' layout
# ----------------------------------------------------------------------------------------------------------------------
def to_rows(t):
    """[B, heads, S, 64] -> [B*S, heads*64] (row = b*S + s, head h at columns h*64 ...), the layout of the HIP ops."""
    B, heads, S, D = t.shape
    return t.permute(0, 2, 1, 3).reshape(B * S, heads * D)


def from_rows(t, B, heads, S):
    return t.reshape(B, S, heads, -1).permute(0, 2, 1, 3)
