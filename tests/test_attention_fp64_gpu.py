"""The attention kernels of csrc/attention.hip against closed-form fp64 attention on the SAME bf16 inputs, on every route the
dispatchers op_attn_fwd / op_attn_bwd can take, at flat and at hard scores (tests/attention_ref.py: families and pad patterns).

Every (sample, head) slice of every launch is checked, per output kind, with the gate of tests/attention_ref.py

    ||got - exact||  <=  MARGINS[kind] * ||model - exact||  +  floor

where `model` is the fp64 computation with the roundings the kernels document and nothing else.  Every launch is made twice and
must return the same bits.  Each case also appends its largest error / model-error ratios to attention_fp64_errors.jsonl in the
tests' output directory (tests/util.py: out_dir()); profiles/attention_fp64_errors_mi355x.jsonl is that record behind MARGINS.

Case ids are built from `routes()`, a mirror of the dispatch rules, so a failing id names its kernels:

  forward   fwd_pers           persistent kernel, 193 ... 257 tokens                       sweep S = 193 250 256 257, families, product
            fwd_res_frag       resident K/V kernel with the fragment-major bias image      sweep S <= 192 and 258 ... 320, families
            fwd_res_nobias     resident kernel without a bias                              families (S = 129), nobias cases
            fwd_stream         streaming kernel: natural above 320 tokens, and forced      sweep S >= 321; families at S = 129
                               (resident knob off / no fragment image) below               (forced) and 449; product at 321, 385
  backward  bwd_persdq_persdkdv   persistent dQ (+ dBias), persistent dK / dV              S = 193 250 257
            bwd_persdq_dkdv       persistent dQ (+ dBias), rounds 1-3 dK / dV kernel       S = 256, and the pers_dkdv knob off
            bwd_mergedN_frag      merged dQ + dBias, N key tiles, fragment image           N = 1 ... 4 (4: persistent kernels off)
            bwd_mergedN_nofrag    ... row-major bias image                                 N = 5, 6 (273 ... 384); 1 ... 4 without an image
            bwd_mergedN_*_tail1   ... last key tile = one 16-key block                     S = 65, 129, 257 (persistent off), 258, 272, 321
            bwd_sep_dbias         separate dQ, dK / dV and dBias kernels                   S >= 385, and the merge knob off
            bwd_sep_nobias        separate dQ and dK / dV kernels, no bias                 nobias cases
            ..._ps                per-sample bias images (merged: slab per sample; separate above 384 tokens / merge knob off)

S = 1 and 2 are supported (every row index of the kernels is clamped to S - 1, stores are guarded by the row count) and run here.
A row with every key masked is NaN in the reference too and is out of scope."""
import json
import os
import time

import pytest
import torch

from tests import attention_ref as R
from tests.util import out_dir

pytestmark = pytest.mark.gpu
DEV = "cuda"


def hipmod():
    from one_peace_amd import hip
    return hip


def cdiv(a, b):
    return (a + b - 1) // b


def routes(S, bias, frag_fwd, frag_bwd, knobs):
    """Mirror of the dispatch in op_attn_fwd / op_attn_bwd (scale 1/8: its inverse is exact in bf16).  bias: None, "shared", "ps"."""
    res, pers, pers_bwd = knobs.get("resident", 1) & 1, knobs.get("attn_pers", 1), knobs.get("attn_pers_bwd", 1)
    merge, pers_dkdv = knobs.get("merge_dbias", 1), knobs.get("attn_pers_dkdv", 1)
    ok_f = bias is None or frag_fwd
    if res and pers and 192 < S <= 257 and ok_f:
        f = "fwd_pers"
    elif res and S <= 320 and ok_f:
        f = "fwd_res_frag" if bias else "fwd_res_nobias"
    else:
        f = "fwd_stream"
    nt = cdiv(S, 64)
    ps = "_ps" if bias == "ps" else ""
    if merge and pers_bwd and 192 < S <= 257 and bias != "ps" and (bias is None or frag_bwd):
        b = "bwd_persdq_" + ("persdkdv" if pers_dkdv and S != 256 else "dkdv") + ("" if bias else "_nobias")
    elif bias and nt <= 6 and merge:
        one_block = cdiv(S - (nt - 1) * 64, 16) == 1
        frag = frag_bwd and (nt <= 4 or (nt == 5 and one_block))
        b = "bwd_merged%d_%s%s%s" % (nt, "frag" if frag else "nofrag", "_tail1" if one_block else "", ps)
    else:
        b = ("bwd_sep_dbias" if bias else "bwd_sep_nobias") + ps
    return f, b


class Case:
    def __init__(self, group, S, B, heads, family="unit", pad="tail", bias="shared", frag_fwd=True, frag_bwd=True, **knobs):
        self.group, self.S, self.B, self.heads, self.family, self.pad, self.bias = group, S, B, heads, family, pad, bias
        self.frag_fwd, self.frag_bwd, self.knobs = bool(bias) and frag_fwd, bool(bias) and frag_bwd, knobs
        self.routes = routes(S, bias, self.frag_fwd, self.frag_bwd, knobs)
        forced = "_forced" if self.routes[0] == "fwd_stream" and S <= 320 else ""
        kn = "".join("-%s%d" % (k, v) for k, v in sorted(knobs.items()))
        self.id = "%s-%s%s-%s-S%d-B%d-h%d-%s-%s%s" % (group, self.routes[0], forced, self.routes[1], S, B, heads, family, pad, kn)


def _cases():
    c = []
    # ---- sweep over S on the default route: peaked scores, ragged tails, B so that the last batch chunk is partial (the merged
    # kernel's chunk rule splits 37 samples of a small launch into 19 chunks of 2 with a last chunk of 1; the persistent dQ kernel
    # 13 x 24 heads into 5 chunks of 3 with a last chunk of 1 -- and 312 items on 256 CUs; the separate kernels 23 samples of
    # 385 tokens x 2 heads into 12 chunks of 2 with a last chunk of 1).  Work-item counts: S = 385 B = 23 h = 2 gives 184
    # workgroups (a multiple of 8: the XCD re-deal), S = 449 B = 5 h = 3 gives 60 (not a multiple: the plain order).
    for S in (1, 2, 16, 17, 63, 64, 65, 129, 192, 193, 250, 256, 258, 272, 273, 320, 384):
        c.append(Case("sweep", S, 37, 2 + S % 2, "peaked", "tail" if S > 1 else "none"))
    c.append(Case("sweep", 257, 13, 24, "peaked", "tail"))
    c.append(Case("sweep", 321, 5, 24, "peaked", "hole"))
    c.append(Case("sweep", 385, 23, 2, "peaked", "tail"))
    c.append(Case("sweep", 449, 5, 3, "peaked", "tail"))
    c.append(Case("sweep", 785, 2, 24, "peaked", "tail"))
    c.append(Case("sweep", 1025, 2, 24, "peaked", "tail"))
    c.append(Case("sweep", 785, 3, 2, "unit", "first_tile", bias="ps"))
    # the merged kernel's remaining tile counts and image forms: 2 full tiles, 4 tiles (the persistent kernels switched off), and the
    # row-major image at 1, 2 and 4 tiles; the resident forward with 16 query blocks
    c.append(Case("sweep", 128, 37, 2, "peaked", "tail"))
    c.append(Case("sweep", 250, 37, 2, "peaked", "tail", attn_pers=0, attn_pers_bwd=0))
    c.append(Case("sweep", 256, 37, 2, "peaked", "tail", attn_pers=0, attn_pers_bwd=0))
    for S in (64, 128, 200):
        c.append(Case("sweep", S, 37, 2, "peaked", "tail", frag_fwd=False, frag_bwd=False))
    # ---- every family on every route, at one S per route
    for fam in R.FAMILIES:
        c.append(Case("families", 257, 5, 3, fam))                                    # persistent forward and backward
        c.append(Case("families", 256, 5, 3, fam))                                    # persistent dQ, rounds 1-3 dK / dV
        c.append(Case("families", 250, 5, 2, fam, attn_pers_dkdv=0))
        c.append(Case("families", 257, 5, 2, fam, attn_pers=0, attn_pers_bwd=0))      # resident (9 query blocks), merged5 frag tail1
        c.append(Case("families", 129, 5, 2, fam))                                    # resident + fragment image, merged3 frag tail1
        c.append(Case("families", 192, 5, 2, fam))                                    # merged3 frag, full tiles
        c.append(Case("families", 129, 5, 2, fam, bias=None))                         # resident without bias, separate dQ
        c.append(Case("families", 129, 5, 2, fam, resident=0))                        # streaming forced, merged frag
        c.append(Case("families", 129, 5, 2, fam, frag_fwd=False, frag_bwd=False))    # streaming (no image), merged nofrag
        c.append(Case("families", 300, 5, 2, fam))                                    # resident, merged5 nofrag
        c.append(Case("families", 321, 5, 2, fam, pad="hole"))                        # streaming natural, merged6 nofrag tail1
        c.append(Case("families", 449, 5, 3, fam))                                    # streaming, separate dQ / dK,dV / dBias
        c.append(Case("families", 129, 5, 2, fam, merge_dbias=0))                     # separate kernels through the knob
        c.append(Case("families", 257, 5, 2, fam, merge_dbias=0))
        c.append(Case("families", 129, 5, 2, fam, bias="ps"))                         # per-sample bias, merged, fragment image
        c.append(Case("families", 129, 5, 2, fam, bias="ps", frag_fwd=False, frag_bwd=False))
        c.append(Case("families", 401, 3, 2, fam, bias="ps"))                         # per-sample bias, separate kernels
        c.append(Case("families", 129, 5, 2, fam, bias="ps", merge_dbias=0))
    # ---- the full family x pad product at the boundary lengths of the routes
    for S in (192, 193, 257, 258, 320, 321, 384, 385):
        for fam in R.FAMILIES:
            for pad in R.PADS:
                c.append(Case("product", S, 3, 2, fam, pad))
    # ---- the streaming route with a middle hole, pads above 384 tokens with a SHARED bias, no bias on the long routes
    c.append(Case("hole", 321, 3, 2, "edge_pad", "hole", resident=0))
    c.append(Case("hole", 449, 3, 2, "edge_pad", "hole"))
    c.append(Case("hole", 785, 2, 3, "winner_late", "hole"))
    c.append(Case("nobias", 257, 7, 3, "peaked", "tail", bias=None))
    c.append(Case("nobias", 321, 3, 2, "peaked", "hole", bias=None))
    c.append(Case("nobias", 785, 2, 2, "ascending", "tail", bias=None))
    ids = [x.id for x in c]
    assert len(set(ids)) == len(ids)
    return c


CASES = _cases()


def _device_inputs(case):
    hip = hipmod()
    B, S, heads = case.B, case.S, case.heads
    pad = R.make_pad(case.pad, B, S)
    assert pad is not None or case.pad == "none"
    q, k, v, bias, dout = R.make_inputs(case.family, B, heads, S, pad, per_sample_bias=case.bias == "ps", use_bias=bool(case.bias))
    q, k, v, dout = (t.to(DEV) for t in (q, k, v, dout))
    bias = bias.to(DEV) if bias is not None else None
    pad = pad.to(DEV) if pad is not None else None
    Spad = hip.attn_spad(S)
    qkv = torch.cat([R.to_rows(t) for t in (q, k, v)], dim=1).to(torch.bfloat16).contiguous()
    dout_d = R.to_rows(dout).to(torch.bfloat16).contiguous()
    bias_d = biasT_d = pad_d = None
    if bias is not None:
        # columns [S, Spad) of the images are unspecified for the kernels: NaN in the query-major image; finite (but absurd) in the
        # key-major one, which the dK / dV kernel adds through the matrix pipe (see include/onepeace_hip.h)
        bias_d = torch.full(bias.shape[:-1] + (Spad,), float("nan"), dtype=torch.bfloat16, device=DEV)
        bias_d[..., :S] = bias.to(torch.bfloat16)
        biasT_d = torch.full_like(bias_d, 3.0e4)
        biasT_d[..., :S] = bias.transpose(-1, -2).to(torch.bfloat16)
    if pad is not None:
        pad_d = torch.ones(B, Spad, dtype=torch.uint8, device=DEV)
        pad_d[:, :S] = pad.to(torch.uint8)
    return (q, k, v, bias, pad, dout), (qkv, dout_d, bias_d, biasT_d, pad_d, Spad)


def _launch(case, dev_in):
    hip = hipmod()
    qkv, dout_d, bias_d, biasT_d, pad_d, Spad = dev_in
    B, S, heads = case.B, case.S, case.heads
    H = heads * 64
    qd, kd, vd = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    frag = hip.attn_bias_pack(bias_d, S) if (case.frag_fwd or case.frag_bwd) else None
    out, lse = hip.attn_fwd(qd, kd, vd, 3 * H, B, S, heads, R.SCALE, bias_d, pad_d, Spad, bias_frag=frag if case.frag_fwd else None)
    dqkv, dbias = hip.attn_bwd(qd, kd, vd, 3 * H, dout_d, out, lse, B, S, heads, R.SCALE, bias_d, biasT_d, pad_d, Spad,
                               want_dbias=bias_d is not None, bias_frag=frag if case.frag_bwd else None)
    return out, lse[:, :, :S].contiguous(), dqkv, (dbias[..., :S].contiguous() if dbias is not None else None)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_attention_against_fp64(case):
    hip = hipmod()
    B, S, heads = case.B, case.S, case.heads
    H = heads * 64
    t0 = time.time()
    ref_in, dev_in = _device_inputs(case)
    saved = {k: getattr(hip.TUNE, k) for k in case.knobs}
    try:
        for k, val in case.knobs.items():
            setattr(hip.TUNE, k, val)
        first = _launch(case, dev_in)
        again = _launch(case, dev_in)
    finally:
        for k, val in saved.items():
            setattr(hip.TUNE, k, val)
    out, lse, dqkv, dbias = first
    got = {"out": R.from_rows(out.double(), B, heads, S), "lse": lse.double(),
           "dq": R.from_rows(dqkv[:, :H].double(), B, heads, S), "dk": R.from_rows(dqkv[:, H:2 * H].double(), B, heads, S),
           "dv": R.from_rows(dqkv[:, 2 * H:].double(), B, heads, S)}
    if dbias is not None:
        got["dbias"] = dbias.double()
    ex = R.attn_exact(*ref_in, R.SCALE)
    md = R.attn_rounding_model(*ref_in, R.SCALE)
    failures, ratios = R.gate(got, ex, md)
    same = all(a is None or torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                                        b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))
               for a, b in zip(first, again))
    finite = {n: bool(torch.isfinite(t).all()) for n, t in got.items()}
    rec = {"case": case.id, "fwd": case.routes[0], "bwd": case.routes[1], "S": S, "B": B, "heads": heads, "family": case.family,
           "pad": case.pad, "ratio": ratios, "finite": all(finite.values()), "repeat_same_bits": same, "gate_failures": len(failures),
           "seconds": round(time.time() - t0, 3)}
    with open(os.path.join(out_dir(), "attention_fp64_errors.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))
    assert all(finite.values()), "non-finite where the exact result is finite: %s" % finite
    assert same, "a repeated launch returned different bits"
    # margins = 1.5 x the measured maxima (tests/attention_ref.py: MEASURED_MAX_RATIO, with what they are made of):
    # out 1.52 (1.011), dq 1.70 (1.131), dk 2.58 (1.722), dv 1.65 (1.101), dbias 1.89 (1.258); lse: the floor alone (<= 0.25 of it)
    assert not failures, "\n".join(failures)

