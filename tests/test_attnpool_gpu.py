"""op_attn_pool_fwd / op_attn_pool_bwd (csrc/attnpool.hip) on the MI355X against fp64: every case of tests/attnpool_ref.py through
gates (a), (b) and (c) with every output in a guarded buffer, run-to-run and batch-independence bit equality, the refusals of the
wrapper and the fallback of ops.attention_pool.  ONEPEACE_ATTNPOOL_RECORD=<file>: the figures of every case are appended to it as
JSON lines (profiles/attn_pool_errors_mi355x.json is such a record)."""
import functools
import json
import os

import pytest
import torch

from tests import attnpool_ref as A

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@functools.lru_cache(maxsize=None)
def _refs(i):
    inp = A.make_inputs(A.CASES[i])
    return inp, A.pool64(inp), A.pool32(inp)


def _launch(case, inp, guarded=True):
    """Both kernels on the case's buffer layout.  Returns (outputs dict, guarded views)."""
    from one_peace_amd import hip
    B, S, H, heads = case.B, case.S, case.H, case.heads
    src = A.plant(inp) if case.layout == "planted" else inp
    k, v = A.lay_out(case, src["k"], src["v"], DEV)
    q = inp["q"].to(DEV, torch.bfloat16)
    dout = inp["dout"].to(DEV, torch.bfloat16)
    pad = inp["pad"].to(DEV) if inp["pad"] is not None else None
    if not guarded:
        out, p = hip.attn_pool_fwd(k, v, q, pad)
        dk, dv, dqp = hip.attn_pool_bwd(dout, k, v, q, p)
        return {"out": out, "p": p, "dk": dk, "dv": dv, "dq": dqp.sum(0).view(heads, case.hd), "dq_part": dqp}, []
    g_out = A.guarded((B * H,), torch.bfloat16, device=DEV)
    g_p = A.guarded((B * heads * S,), torch.float32, device=DEV)
    g_dk = A.guarded((B * S, H), torch.bfloat16, device=DEV)     # row stride H + 8: the gradients' own ldg / batch stride
    g_dv = A.guarded((B * S, H), torch.bfloat16, device=DEV)
    g_dq = A.guarded((B * H,), torch.float32, device=DEV)
    ldg = g_dk.stride(0)
    dk = g_dk.as_strided((B, S, H), (S * ldg, ldg, 1), g_dk.storage_offset())
    dv = g_dv.as_strided((B, S, H), (S * ldg, ldg, 1), g_dv.storage_offset())
    out, p = hip.attn_pool_fwd(k, v, q, pad, out=g_out.view(B, H), p=g_p.view(B, heads, S))
    hip.attn_pool_bwd(dout, k, v, q, p, dk=dk, dv=dv, dq_part=g_dq.view(B, H))
    torch.cuda.synchronize()
    return ({"out": out, "p": p, "dk": dk, "dv": dv, "dq": g_dq.view(B, H).sum(0).view(heads, case.hd), "dq_part": g_dq.view(B, H)},
            [("out", g_out), ("p", g_p), ("dk", g_dk), ("dv", g_dv), ("dq_part", g_dq)])


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=[c.id for c in A.CASES])
def test_kernels_meet_the_gates(i):
    case = A.CASES[i]
    inp, y64, y32 = _refs(i)
    got, guards = _launch(case, inp)
    for name, view in guards:
        assert A.check_guard(view) == 0, "%s: %d guard elements overwritten" % (name, A.check_guard(view))
    ref16 = A.pool_refarith(inp, torch.bfloat16, DEV)
    fails, fig = A.gate(case, got, y64, y32, ref16)
    print(case.id, json.dumps(fig))
    rec = os.environ.get("ONEPEACE_ATTNPOOL_RECORD")
    if rec:
        with open(rec, "a") as f:
            f.write(json.dumps({"case": case.id, "figures": fig, "failures": fails}) + "\n")
    assert not fails, fails
    if inp["pad"] is not None:   # masked keys: p = 0 exactly and zero gradient rows, also under the planted Inf / NaN
        m = inp["pad"].to(DEV)
        assert int((got["p"] != 0)[m[:, None, :].expand_as(got["p"])].sum()) == 0
        assert int((got["dk"] != 0)[m].sum()) == 0 and int((got["dv"] != 0)[m].sum()) == 0


def test_two_runs_are_bit_identical():
    for i in (2, 5, 7):
        case = A.CASES[i]
        inp = _refs(i)[0]
        a, _ = _launch(case, inp, guarded=False)
        b, _ = _launch(case, inp, guarded=False)
        for name in a:
            assert torch.equal(a[name].view(torch.int16 if a[name].dtype == torch.bfloat16 else torch.int32),
                               b[name].view(torch.int16 if b[name].dtype == torch.bfloat16 else torch.int32)), (case.id, name)


def test_a_sample_does_not_depend_on_its_batch():
    """Row b of the B = 5 launch equals the B = 1 launch of that sample bit for bit (dq: the per-sample partial)."""
    i = 2
    case = A.CASES[i]
    assert case.B == 5
    inp = _refs(i)[0]
    full, _ = _launch(case, inp, guarded=False)
    for b in range(case.B):
        one = {n: (t[b:b + 1] if n != "q" and t is not None else t) for n, t in inp.items()}
        c1 = A.Case(1, case.S, case.heads, case.hd, case.mask, case.layout, case.qscale)
        got, _ = _launch(c1, one, guarded=False)
        for name in ("out", "p", "dk", "dv", "dq_part"):
            x, y = full[name][b:b + 1].contiguous(), got[name].contiguous()
            it = torch.int16 if x.dtype == torch.bfloat16 else torch.int32
            assert torch.equal(x.view(it), y.view(it)), (b, name)


def test_out_of_limit_shapes_raise_and_the_op_falls_back():
    from one_peace_amd import hip, ops
    mk = lambda *s: torch.randn(*s, device=DEV).to(torch.bfloat16)  # noqa: E731
    bad = [(mk(2, 7, 24), mk(2, 7, 24), mk(2, 12)),                               # hd = 12
           (mk(1, 4097, 16), mk(1, 4097, 16), mk(2, 8)),                          # S = 4097
           (mk(2, 7, 129)[:, :, :128], mk(2, 7, 129)[:, :, :128], mk(2, 64))]     # odd ld
    for k, v, q in bad:
        with pytest.raises(RuntimeError):
            hip.attn_pool_fwd(k, v, q)
        p = torch.zeros(k.shape[0], q.shape[0], k.shape[1], device=DEV)
        with pytest.raises(RuntimeError):
            hip.attn_pool_bwd(mk(k.shape[0], k.shape[2]), k, v, q, p)
        calls = []
        orig = hip.attn_pool_fwd
        hip.attn_pool_fwd = lambda *a, **kw: calls.append(1) or orig(*a, **kw)
        try:
            kk = k.detach().requires_grad_(True)
            out = ops.attention_pool(kk, v, q)
            out.float().sum().backward()
        finally:
            hip.attn_pool_fwd = orig
        assert not calls and out.shape == (k.shape[0], k.shape[2]) and kk.grad is not None
        want = ops.attention_pool_torch(k, v, q)
        assert torch.equal(out, want)


def test_autograd_function_runs_the_kernels():
    """ops.attention_pool on bf16 device tensors calls both wrappers and returns their results (q as the reference's parameter)."""
    from one_peace_amd import hip, ops
    i = 1
    case = A.CASES[i]
    inp, y64, y32 = _refs(i)
    k, v = A.lay_out(case, inp["k"], inp["v"], DEV)
    k.requires_grad_(True)
    v.requires_grad_(True)
    q = inp["q"].to(DEV, torch.bfloat16).view(1, 1, case.heads, case.hd).requires_grad_(True)
    calls = []
    of, ob = hip.attn_pool_fwd, hip.attn_pool_bwd
    hip.attn_pool_fwd = lambda *a, **kw: calls.append("fwd") or of(*a, **kw)
    hip.attn_pool_bwd = lambda *a, **kw: calls.append("bwd") or ob(*a, **kw)
    try:
        out = ops.attention_pool(k, v, q, inp["pad"].to(DEV))
        out.backward(inp["dout"].to(DEV, torch.bfloat16))
    finally:
        hip.attn_pool_fwd, hip.attn_pool_bwd = of, ob
    assert calls == ["fwd", "bwd"]
    got = {"out": out, "dk": k.grad, "dv": v.grad}
    fails, _ = A.gate(case, got, y64, y32, names=("out", "dk", "dv"))
    assert not fails, fails
    # dq arrives in the parameter's dtype: the fp32 sum rounded to bf16 once
    err = (q.grad.double().cpu().view(case.heads, case.hd) - y64["dq"]).abs()
    assert bool((err <= A.U16 * y64["dq"].abs() + A.e32(case, "dq", y64, y32)).all())
