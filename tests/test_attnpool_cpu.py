"""tests/attnpool_ref.py and the torch fallback of ops.attention_pool, checked without a GPU: the fallback meets gates (a) and (b)
against fp64 on every case, every mutant of the fp64 computation is rejected by the gates, the fp32 restatement agrees with the fp64
statement, and -- where the reference tree is present -- the reference-arithmetic statement and ops.attention_pool_torch equal the
unmodified MultiheadAttentionPooling bit for bit in fp32 and in bf16."""
import functools
import os
import shutil
import subprocess
import sys

import pytest
import torch

from oracle import ref_shim
from tests import attnpool_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in A.CASES if c.B * c.S * c.H <= 400000]   # the mutant sweep needs no large case


@functools.lru_cache(maxsize=None)
def _refs(i):
    inp = A.make_inputs(A.CASES[i])
    return inp, A.pool64(inp), A.pool32(inp)


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=[c.id for c in A.CASES])
def test_torch_fallback_meets_the_gates(i):
    """fp32 CPU tensors run the torch statement through ops.attention_pool, gradients by autograd.  The inputs carry no planted
    Inf / NaN: the torch statement multiplies masked rows by zero as the reference does (the kernels' skip is the documented deviation)."""
    from one_peace_amd import ops
    case = A.CASES[i]
    inp, y64, y32 = _refs(i)
    k, v = A.lay_out(case, inp["k"], inp["v"], "cpu", torch.float32)
    k.requires_grad_(True)
    v.requires_grad_(True)
    q = inp["q"].clone().view(1, 1, case.heads, case.hd).requires_grad_(True)   # the reference's parameter shape
    out = ops.attention_pool(k, v, q, inp["pad"])
    assert out.shape == (case.B, case.H) and out.dtype == torch.float32
    out.backward(inp["dout"])
    _, pf = A.refarith_forward(k.detach(), v.detach(), q.detach(), inp["pad"])
    got = {"out": out, "p": pf.view(case.B, case.heads, case.S), "dk": k.grad, "dv": v.grad, "dq": q.grad.view(case.heads, case.hd)}
    fails, fig = A.gate(case, got, y64, y32)
    print(case.id, {n: "%.3g" % f["ratio"] for n, f in fig.items()})
    assert not fails, fails


@pytest.mark.parametrize("i", range(len(A.CASES)), ids=[c.id for c in A.CASES])
def test_fp32_restatement_is_an_fp32_computation(i):
    """pool32 (the kernel's hand-derived formulae) agrees with the autograd fp64 statement to fp32 accuracy: per tensor within
    64 (S + hd) 2^-24 of the tensor's largest value -- the formulae are right, and E32 is a small number, not a loophole."""
    case = A.CASES[i]
    _, y64, y32 = _refs(i)
    for name in A.BF16_OUTPUTS + A.F32_OUTPUTS:
        err = float((y32[name].double() - y64[name]).abs().max())
        scale = float(y64[name].abs().max())
        qk = max(1.0, 8.0 * case.qscale)   # the scores' size: an fp32 score error of |s| 2^-24 becomes a relative error of p
        assert err <= 64 * qk * (case.S + case.hd) * A.U32 * scale, (name, err, scale)


@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    """A kernel with that bug, even one exact in fp64, fails the gates on at least one small case (masked cases for the mask mutants)."""
    rejected = []
    for case in SMALL:
        if case.S < 2 or (mutant == "mask_ignored" and case.mask == "none") or (mutant == "head_offset_dropped" and case.heads < 2):
            continue
        inp, y64, y32 = _refs(A.CASES.index(case))
        bad = A.pool64(inp, mutant)
        fails, _ = A.gate(case, bad, y64, y32)
        if fails:
            rejected.append(case.id)
        if mutant != "last_key_dropped":   # (the last key of a right-padded row is masked already: only some cases can show it)
            assert fails, "%s passes the gates on %s" % (mutant, case.id)
    assert rejected, "%s passes the gates on every case" % mutant


def test_gate_accepts_the_exact_result_rounded_once():
    for i, case in enumerate(A.CASES[:6]):
        inp, y64, y32 = _refs(i)
        got = {n: (A.bf(y64[n].float()) if n in A.BF16_OUTPUTS else y64[n].float()) for n in y64}
        fails, _ = A.gate(case, got, y64, y32)
        assert not fails, fails


def test_all_keys_masked_gives_nan_and_out_of_limit_shapes_fall_back():
    from one_peace_amd import hip, ops
    k, v, q = torch.randn(2, 5, 16), torch.randn(2, 5, 16), torch.randn(2, 8)
    pad = torch.zeros(2, 5, dtype=torch.bool)
    pad[1] = True
    out = ops.attention_pool(k, v, q, pad)
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isnan(out[1]).all())
    # the limits of the kernels, as the Python side states them (no device needed)
    mk = lambda B, S, H: torch.empty(B, S, H, dtype=torch.bfloat16)  # noqa: E731
    assert hip.attn_pool_supported(mk(2, 7, 128), mk(2, 7, 128), 2, 64)
    assert hip.attn_pool_supported(mk(2, 8, 128)[:, 1:], mk(2, 8, 128)[:, 1:], 2, 64)
    assert not hip.attn_pool_supported(mk(2, 7, 24), mk(2, 7, 24), 2, 12)            # hd % 8
    assert not hip.attn_pool_supported(mk(1, 4097, 16), mk(1, 4097, 16), 2, 8)       # S
    assert not hip.attn_pool_supported(mk(2, 7, 272), mk(2, 7, 272), 2, 136)         # hd > 128
    assert not hip.attn_pool_supported(mk(2, 7, 129)[:, :, :128], mk(2, 7, 129)[:, :, :128], 2, 64)   # odd ld
    with pytest.raises(ValueError):
        ops.attention_pool(k, v, torch.randn(3, 8))


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
def test_kernels_compile_without_scratch_without_atomics_and_with_16_byte_loads(tmp_path):
    sys.path.insert(0, ROOT)
    from tools import check_mfma_hazards as C
    isa = C.compile_isa(str(tmp_path), "attnpool")
    usage = C.resource_usage(isa)
    for kernel in ("attn_pool_fwd_kernel", "attn_pool_bwd_kernel"):   # one instantiation per group width 1, 2, 4, 8, 16
        assert sum(kernel in n for n in usage) == 5, (kernel, sorted(usage))
    assert len(usage) == 10 and all(u.get("ScratchSize", 1) == 0 for u in usage.values()), usage
    text = open(isa).read()
    assert "atomic" not in text and "ds_add_f" not in text
    assert "global_load_dwordx4" in text and "global_store_dwordx4" in text   # 16-byte loads of k / v, 16-byte stores of dk / dv


@pytest.mark.skipif(not ref_shim.reference_available(), reason="reference tree not present")
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_reference_arithmetic_equals_the_unmodified_module(dtype):
    """tests/attnpool_ref.py: check_against_reference_module, in a child process -- loading the reference through oracle/ref_shim.py
    puts stand-ins for fairseq into sys.modules, which must not leak into the other tests of this process."""
    r = subprocess.run([sys.executable, "-m", "tests.attnpool_ref", dtype], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "equal on" in r.stdout, r.stdout[-3000:]
