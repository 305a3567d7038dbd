"""Shared by tests/test_attnpool_cpu.py and tests/test_attnpool_gpu.py: single-query attention pooling (csrc/attnpool.hip,
ops.attention_pool) stated three ways, the case list, the gates and mutants of the fp64 computation.  Nothing here needs a GPU.

    pool64      the fp64 statement: masked softmax of q_h . k_s WITHOUT 1 / sqrt(hd), the weighted sum of v, and its gradients by
                autograd under the cotangent dout.  Masked rows of k and v are not read (the op's documented deviation from the
                reference, whose bmm multiplies them by zero).
    pool32      the kernel's formula restated in fp32 on the CPU, outputs NOT rounded: what fp32 arithmetic alone costs on the case.
    pool_refarith  one_peace_base.py:154-170 at the input dtype (bmm, masked_fill_(-inf), softmax(dtype=float32), type_as, bmm) with
                autograd: what the op replaces.

Every input holds bf16 VALUES, so all three and a kernel see the same numbers.  Outputs, as a dict: out [B, H], p [B, heads, S],
dk, dv [B, S, H], dq [heads, hd] (summed over the batch).

Gates of one output tensor against y64 = pool64 (gate()):
  (a) bf16 outputs (out, dk, dv), per element:  |got - y64| <= 2^-8 |y64| + E32.  2^-8: the unit roundoff of the one bf16 rounding.
  (b) fp32 outputs (p, dq), per tensor:         max |got - y64| <= E32.
  (c) per tensor: max |got - y64| <= max |pool_refarith(bf16) - y64| -- the op is not less accurate than what it replaces (skipped
      where the reference's own result is not finite: planted Inf / NaN in masked rows).
E32 = max(4 max |pool32 - y64|, (S + hd) 2^-24 max |y64|), per case and tensor: 4 covers another summation order and a device expf
that is one ulp off; the floor is one fp32 rounding per term of the longest sums, for cases where pool32 happens to be exact (S = 1)."""
import math

import torch

from tests.gemm_ref import check_guard, guarded, half_ulp_bf16  # noqa: F401  (re-exported for the two test files)

U32 = 2.0 ** -24
U16 = 2.0 ** -8
BF16_OUTPUTS = ("out", "dk", "dv")
F32_OUTPUTS = ("p", "dq")
MUTANTS = ("last_key_dropped", "mask_ignored", "scaled_by_rsqrt_hd", "v_taken_from_k", "head_offset_dropped", "c_omitted_in_ds")


class Case:
    def __init__(self, B, S, heads, hd, mask, layout, qscale=1.0):
        self.B, self.S, self.heads, self.hd, self.mask, self.layout, self.qscale = B, S, heads, hd, mask, layout, qscale
        self.H = heads * hd
        self.id = "B%d-S%d-h%d-d%d-%s-%s%s" % (B, S, heads, hd, mask, layout, "" if qscale == 1.0 else "-q%g" % qscale)


# mask: none | right (another length per row; row 0 full, row 1 exactly one live key) | alternate (every second key masked)
# layout: plain | halves (k, v = the halves of one [B, S, 2 H] buffer) | slice ([:, 1:] of [B, S + 1, H]) | planted (plain, +Inf in the
#         masked rows of v and NaN in the masked rows of k)
CASES = [
    Case(3, 1, 2, 64, "none", "plain"),
    Case(4, 7, 2, 64, "right", "halves"),
    Case(5, 65, 3, 64, "alternate", "slice"),
    Case(4, 256, 2, 64, "none", "plain"),
    Case(4, 257, 2, 64, "right", "planted"),
    Case(3, 749, 2, 64, "alternate", "halves", qscale=0.25),
    Case(2, 1024, 24, 64, "right", "plain"),
    Case(4, 300, 2, 64, "right", "slice", qscale=4.0),   # hard scores: q . k ~ N(0, 32^2), the softmax close to one-hot
    Case(4, 130, 4, 32, "alternate", "planted"),
    Case(2, 70, 1, 128, "right", "halves"),
]


def bf(x):
    return x.to(torch.bfloat16).to(x.dtype)


def make_inputs(case, seed=0):
    """CPU fp32 tensors of bf16 values: k, v [B, S, H], q [heads, hd], dout [B, H] ~ N(0, 1) (q times qscale); pad bool [B, S] | None."""
    g = torch.Generator().manual_seed(7000 + 31 * seed + CASES.index(case) if case in CASES else seed)
    B, S, H = case.B, case.S, case.H
    k, v = bf(torch.randn(B, S, H, generator=g)), bf(torch.randn(B, S, H, generator=g))
    q = bf(torch.randn(case.heads, case.hd, generator=g) * case.qscale)
    dout = bf(torch.randn(B, H, generator=g))
    pad = None
    if case.mask == "right":
        lens = torch.randint(1, S + 1, (B,), generator=g)
        lens[0] = S
        if B > 1:
            lens[1] = 1
        pad = torch.arange(S)[None, :] >= lens[:, None]
    elif case.mask == "alternate":
        pad = (torch.arange(S) % 2 == 1)[None, :].expand(B, S).contiguous()
    return {"k": k, "v": v, "q": q, "dout": dout, "pad": pad}


def plant(inp):
    """+Inf in the masked rows of v, NaN in the masked rows of k (layout "planted")."""
    out = dict(inp)
    m = inp["pad"][:, :, None]
    out["v"] = torch.where(m, torch.full_like(inp["v"], float("inf")), inp["v"])
    out["k"] = torch.where(m, torch.full_like(inp["k"], float("nan")), inp["k"])
    return out


def lay_out(case, k, v, device, dtype=torch.bfloat16):
    """k, v as `dtype` views on `device` in the case's buffer layout; whatever the views do not cover is NaN."""
    B, S, H = k.shape
    if case.layout == "halves":
        buf = torch.full((B, S, 2 * H), float("nan"), dtype=dtype, device=device)
        kk, vv = buf[:, :, :H], buf[:, :, H:]
    elif case.layout == "slice":
        kk = torch.full((B, S + 1, H), float("nan"), dtype=dtype, device=device)[:, 1:]
        vv = torch.full((B, S + 1, H), float("nan"), dtype=dtype, device=device)[:, 1:]
    else:
        kk, vv = torch.empty(B, S, H, dtype=dtype, device=device), torch.empty(B, S, H, dtype=dtype, device=device)
    kk.copy_(k)
    vv.copy_(v)
    return kk, vv


def _unmasked(t, pad):
    return t if pad is None else torch.where(pad[:, :, None], torch.zeros_like(t), t)


def pool64(inp, mutant=None):
    assert mutant is None or mutant in MUTANTS, mutant
    pad = inp["pad"]
    heads, hd = inp["q"].shape
    if mutant == "mask_ignored":
        pad = None
    if mutant == "last_key_dropped":
        last = torch.zeros(inp["k"].shape[:2], dtype=torch.bool)
        last[:, -1] = True
        pad = last if pad is None else pad | last
    k = _unmasked(inp["k"].double(), pad).requires_grad_(True)
    v = _unmasked(inp["v"].double(), pad).requires_grad_(True)
    q = inp["q"].double().requires_grad_(True)
    dout = inp["dout"].double()
    B, S, H = k.shape
    k4, v4 = k.view(B, S, heads, hd), (k if mutant == "v_taken_from_k" else v).view(B, S, heads, hd)
    if mutant == "head_offset_dropped":
        k4, v4 = k4[:, :, :1].expand(B, S, heads, hd), v4[:, :, :1].expand(B, S, heads, hd)
    s = torch.einsum("bshd,hd->bhs", k4, q)
    if mutant == "scaled_by_rsqrt_hd":
        s = s * hd ** -0.5
    if pad is not None:
        s = s.masked_fill(pad[:, None, :], -math.inf)
    p = torch.softmax(s, dim=-1)
    out = torch.einsum("bhs,bshd->bhd", p, v4).reshape(B, H)
    dk, dv, dq = torch.autograd.grad(out, (k, v, q), dout, allow_unused=True)
    dv = torch.zeros_like(v) if dv is None else dv
    if mutant == "c_omitted_in_ds":
        pd = p.detach()
        ds = pd * torch.einsum("bhd,bshd->bhs", dout.view(B, heads, hd), v4.detach())
        dk = torch.einsum("bhs,hd->bshd", ds, q.detach()).reshape(B, S, H)
        dq = torch.einsum("bhs,bshd->hd", ds, k4.detach())
    return {"out": out.detach(), "p": p.detach(), "dk": dk, "dv": dv, "dq": dq}


def pool32(inp):
    """The kernel's formula in fp32 (CPU), outputs unrounded."""
    pad = inp["pad"]
    heads, hd = inp["q"].shape
    k, v = _unmasked(inp["k"].float(), pad), _unmasked(inp["v"].float(), pad)
    q, dout = inp["q"].float(), inp["dout"].float()
    B, S, H = k.shape
    k4, v4, g = k.view(B, S, heads, hd), v.view(B, S, heads, hd), dout.view(B, heads, hd)
    s = torch.einsum("bshd,hd->bhs", k4, q)
    if pad is not None:
        s = s.masked_fill(pad[:, None, :], -math.inf)
    e = torch.exp(s - s.max(dim=-1, keepdim=True)[0])
    p = e / e.sum(dim=-1, keepdim=True)
    out = torch.einsum("bhs,bshd->bhd", p, v4).reshape(B, H)
    dp = torch.einsum("bhd,bshd->bhs", g, v4)
    c = (p * dp).sum(dim=-1, keepdim=True)
    ds = p * (dp - c)
    dv = torch.einsum("bhs,bhd->bshd", p, g).reshape(B, S, H)
    dk = torch.einsum("bhs,hd->bshd", ds, q).reshape(B, S, H)
    dq = torch.einsum("bhs,bshd->hd", ds, k4)
    return {"out": out, "p": p, "dk": dk, "dv": dv, "dq": dq}


def refarith_forward(k, v, q, pad):
    """one_peace_base.py:154-170 between the projections, op for op: k, v [B, S, H] (any strides), q [1, 1, heads, hd], pad bool [B, S]
    | None.  Returns (attn [B, H], attn_weights_float [B, heads, 1, S])."""
    B, S, H = k.shape
    heads, hd = q.shape[-2], q.shape[-1]
    kt, vt = k.transpose(0, 1).contiguous(), v.transpose(0, 1).contiguous()   # what k_proj / v_proj return for a time-major x
    q = q.expand(1, B, -1, -1).reshape(1, B * heads, hd).transpose(0, 1)
    kk = kt.view(S, B * heads, hd).transpose(0, 1)
    vv = vt.view(S, B * heads, hd).transpose(0, 1)
    attn_weights = torch.bmm(q, kk.transpose(1, 2))
    attn_weights = attn_weights.view(B, heads, 1, S)
    if pad is not None:
        key_padding_mask = pad.view(B, 1, 1, S).contiguous()
        attn_weights.masked_fill_(key_padding_mask.expand(B, heads, 1, S), -math.inf)
    attn_weights_float = torch.nn.functional.softmax(attn_weights, dim=-1, dtype=torch.float32)
    attn_probs = attn_weights_float.type_as(attn_weights)
    attn_probs = attn_probs.view(B * heads, 1, S)
    attn = torch.bmm(attn_probs, vv)
    return attn.reshape(B, H), attn_weights_float


def pool_refarith(inp, dtype, device="cpu"):
    """The reference's arithmetic at `dtype` with autograd (same dict of outputs; p is its fp32 softmax)."""
    pad = inp["pad"].to(device) if inp["pad"] is not None else None
    heads, hd = inp["q"].shape
    k = inp["k"].to(device=device, dtype=dtype).requires_grad_(True)
    v = inp["v"].to(device=device, dtype=dtype).requires_grad_(True)
    q = inp["q"].to(device=device, dtype=dtype).view(1, 1, heads, hd).requires_grad_(True)
    attn, pf = refarith_forward(k, v, q, pad)
    attn.backward(inp["dout"].to(device=device, dtype=dtype))
    return {"out": attn.detach(), "p": pf.detach().view(k.shape[0], heads, -1), "dk": k.grad, "dv": v.grad, "dq": q.grad.view(heads, hd)}


def _maxerr(got, want):
    e = (got.detach().double().cpu() - want).abs()
    return float("inf") if not bool(torch.isfinite(e).all()) else float(e.max())


def e32(case, name, y64, y32):
    """The fp32 allowance of one tensor of one case."""
    m = float(y64[name].abs().max())
    return max(4.0 * _maxerr(y32[name], y64[name]), (case.S + case.hd) * U32 * m)


def gate(case, got, y64, y32, ref16=None, names=BF16_OUTPUTS + F32_OUTPUTS):
    """(failures, figures).  got: name -> tensor (any device / dtype).  figures: name -> {"err", "e32", "ratio" = what the gate of that
    tensor used over what it allows (<= 1 passes), "ref_err" when ref16 is given}."""
    fails, fig = [], {}
    for name in names:
        want = y64[name]
        g = got[name].detach().double().cpu().reshape(want.shape)
        allow32 = e32(case, name, y64, y32)
        if not bool(torch.isfinite(g).all()):
            fails.append("%s: %d non-finite elements" % (name, int((~torch.isfinite(g)).sum())))
            fig[name] = {"err": float("inf"), "e32": allow32, "ratio": float("inf")}
            continue
        err = (g - want).abs()
        bound = U16 * want.abs() + allow32 if name in BF16_OUTPUTS else torch.full_like(want, allow32)
        rel = torch.where(err > 0, err / bound, torch.zeros_like(err))   # (an exact zero against a zero bound, S = 1, is a pass)
        ratio = float(rel.max())
        fig[name] = {"err": float(err.max()), "e32": allow32, "ratio": ratio}
        if ratio > 1.0:
            i = tuple(rel.flatten().argmax().reshape(1).tolist())
            fails.append("%s (%s): |got - fp64| = %.3e exceeds %.3e at flat index %d (E32 %.3e; %d of %d elements)" % (
                name, "a" if name in BF16_OUTPUTS else "b", float(err.flatten()[i[0]]), float(bound.flatten()[i[0]]), i[0], allow32,
                int((err > bound).sum()), err.numel()))
        if ref16 is not None:
            ref_err = _maxerr(ref16[name], want)
            fig[name]["ref_err"] = ref_err
            if float(err.max()) > ref_err:
                fails.append("%s (c): max error %.3e above the reference arithmetic's %.3e" % (name, float(err.max()), ref_err))
    return fails, fig


def check_against_reference_module(dtype):
    """The UNMODIFIED MultiheadAttentionPooling (through oracle/ref_shim.py) with identity projections -- exact in every dtype: one
    product by 1 and sums of zeros -- computes exactly lines 154-170.  refarith_forward and ops.attention_pool_torch must reproduce
    its output and its gradients bit for bit.  Run in a process of its own (python -m tests.attnpool_ref fp32|bf16): the shim puts
    stand-ins for fairseq into sys.modules.  Returns the ids of the cases checked."""
    from one_peace_amd import ops
    from oracle import ref_shim
    base = ref_shim.ref("one_peace.models.one_peace.one_peace_base")
    done = []
    for case in [c for c in CASES if c.mask != "none" and c.B * c.S * c.H <= 400000]:
        inp = make_inputs(case)
        m = base.MultiheadAttentionPooling(case.H, case.heads)
        with torch.no_grad():
            for lin in (m.k_proj, m.v_proj, m.out_proj):
                lin.weight.copy_(torch.eye(case.H))
                if lin.bias is not None:
                    lin.bias.zero_()
            m.q.copy_(inp["q"].view(1, 1, case.heads, case.hd))
        m = m.to(dtype)
        x = inp["k"].to(dtype).clone().requires_grad_(True)   # identity projections: k = v = x
        want = m(x, inp["pad"])
        want.backward(inp["dout"].to(dtype))
        for fn in (lambda k, v, q, pad: refarith_forward(k, v, q, pad)[0], ops.attention_pool_torch):
            k = inp["k"].to(dtype).clone().requires_grad_(True)
            v = inp["k"].to(dtype).clone().requires_grad_(True)
            q = inp["q"].to(dtype).clone().view(1, 1, case.heads, case.hd).requires_grad_(True)
            got = fn(k, v, q, inp["pad"])
            got.backward(inp["dout"].to(dtype))
            assert torch.equal(got, want), case.id
            assert torch.equal(q.grad, m.q.grad), case.id
            if dtype == torch.float32:   # x.grad = dk + dv: one fp32 addition either way
                assert torch.equal(k.grad + v.grad, x.grad), case.id
        done.append(case.id)
    return done


if __name__ == "__main__":
    import sys
    ids = check_against_reference_module({"fp32": torch.float32, "bf16": torch.bfloat16}[sys.argv[1]])
    print("equal on", len(ids), "cases:", " ".join(ids))
