"""Coherence of the derived weight copies of the fp8 input-gradient GEMMs (ops._transposed -> ops._fp8_derived), no GPU: the two ctypes
wrappers that write them (transpose, quant_fp8_rows) are replaced by torch stand-ins that, like the kernels, write through the buffer
without bumping its _version.  After every kind of weight update the fp8 copy must be the quantisation of the CURRENT weights, written
into the same (q, scale) buffers (a captured TrainStepGraph reads them by address), and an unchanged weight must cost no quantisation."""
import pytest
import torch

from one_peace_amd import hip, ops


def _quant_ref(x):
    amax = x.float().abs().amax(dim=1)
    s = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (x.float() / s[:, None]).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8), s


def _transpose_ref(w, scale=None):
    y = w.detach() if scale is None else (w.detach().float() * scale.detach().float()[:, None]).to(w.dtype)
    return y.t().contiguous()


class _Kernels:
    """Stand-ins for hip.transpose / transpose_table / transpose_batched / quant_fp8_rows; counts the quantisations."""

    def __init__(self, monkeypatch):
        self.quants = 0
        monkeypatch.setattr(hip, "quant_fp8_rows", self.quant)
        monkeypatch.setattr(hip, "transpose", self.transpose)
        monkeypatch.setattr(hip, "transpose_table", lambda jobs, device: (list(jobs), 0))
        monkeypatch.setattr(hip, "transpose_batched", self.transpose_batched)
        for name in ("_wt_cache", "_fp8_cache", "_fp8_pairs", "_fp8_derived_cache"):
            monkeypatch.setattr(ops, name, {})
        monkeypatch.setattr(ops, "_refresh_plan", None)
        monkeypatch.setattr(ops, "FP8_FFN", True)

    def quant(self, x, out=None):
        self.quants += 1
        q, s = _quant_ref(x)
        if out is None:
            return q.clone(), s.clone()
        out[0].data.copy_(q)  # .data: a raw write, the buffer's _version stays
        out[1].data.copy_(s)
        return out

    @staticmethod
    def transpose(x, out=None, scale=None):
        y = _transpose_ref(x, scale)
        if out is None:
            return y
        out.data.copy_(y)
        return out

    @staticmethod
    def transpose_batched(jobs, n, tiles):
        assert len(jobs) == n
        for src, dst, scale in jobs:
            dst.data.copy_(_transpose_ref(src, scale))


class _Layer(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.w = torch.nn.Parameter((torch.randn(48, 32, generator=g) * 0.1).to(torch.bfloat16))
        self.g2 = torch.nn.Parameter((1e-2 * (1 + torch.rand(48, generator=g))).to(torch.bfloat16))


def _raw_write(p, value):
    p.data.copy_(value)  # like the fused AdamW kernel: new values, no _version bump


def _update(kind, m, other, ops_):
    g = torch.Generator().manual_seed(7)
    with torch.no_grad():
        if kind == "mul_":
            m.w.mul_(-1)
        elif kind == "optimizer":
            m.w.grad = torch.randn(m.w.shape, generator=g).to(torch.bfloat16)
            m.g2.grad = torch.randn(m.g2.shape, generator=g).to(torch.bfloat16) * 1e-3
            torch.optim.SGD(m.parameters(), lr=0.5).step()
        elif kind == "load_state_dict":
            m.load_state_dict(other.state_dict())
        elif kind == "data":
            m.w.data = other.w.detach().clone()
        elif kind == "gamma":
            m.g2.mul_(3)
        elif kind == "invalidate":
            _raw_write(m.w, other.w)
            _raw_write(m.g2, other.g2)
            ops_.invalidate_weight_cache()
        elif kind == "refresh":
            _raw_write(m.w, other.w)
            _raw_write(m.g2, other.g2)
            ops_.refresh_weight_cache()
        else:
            raise AssertionError(kind)


def _check_current(m, scaled, t, qs):
    want_t = _transpose_ref(m.w, m.g2 if scaled else None)
    assert torch.equal(t, want_t), "stale transposed bf16 copy"
    want_q, want_s = _quant_ref(want_t)
    assert torch.equal(qs[0], want_q) and torch.equal(qs[1], want_s), "stale fp8 copy of the transposed weight"


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("kind", ["mul_", "optimizer", "load_state_dict", "data", "gamma", "invalidate", "refresh"])
def test_fp8_copy_follows_every_kind_of_weight_update(monkeypatch, kind, scaled):
    k = _Kernels(monkeypatch)
    m, other = _Layer(1), _Layer(2)

    def derived():
        t = ops._transposed(m.w, scale=m.g2 if scaled else None)
        return t, ops._fp8_derived(t)

    t0, qs0 = derived()
    _check_current(m, scaled, t0, qs0)
    addr = (qs0[0].data_ptr(), qs0[1].data_ptr())
    n = k.quants
    t1, qs1 = derived()
    assert k.quants == n and t1 is t0 and qs1 is qs0, "an unchanged weight must not be quantised again"

    _update(kind, m, other, ops)
    t2, qs2 = derived()
    _check_current(m, scaled, t2, qs2)
    assert (qs2[0].data_ptr(), qs2[1].data_ptr()) == addr, "re-quantisation must write into the same buffers"
    changed = kind != "gamma" or scaled  # gamma is folded into the scaled copy only
    assert k.quants == n + changed, "one quantisation per update, none without one"
    n = k.quants
    t3, qs3 = derived()
    assert k.quants == n and qs3 is qs2 and t3 is t2


def test_refresh_before_first_use_after_update_costs_no_second_quantisation(monkeypatch):
    """refresh_weight_cache re-quantises every derived entry in its batch: the next backward finds them current."""
    k = _Kernels(monkeypatch)
    m, other = _Layer(1), _Layer(2)
    t = ops._transposed(m.w, scale=m.g2)
    qs = ops._fp8_derived(t)
    with torch.no_grad():
        m.w.mul_(2)  # a version bump AND a refresh (an optimiser step through torch followed by the project's refresh)
    ops.refresh_weight_cache()
    n = k.quants
    assert ops._fp8_derived(ops._transposed(m.w, scale=m.g2)) is qs and k.quants == n
    _check_current(m, True, t, qs)


def test_eviction_above_4096_entries_keeps_live_buffers(monkeypatch):
    k = _Kernels(monkeypatch)
    live = [torch.full((1, 8), float(i + 1), dtype=torch.bfloat16) for i in range(4000)]
    first = [ops._fp8_derived(t) for t in live]
    dead = [torch.full((2, 8), float(i + 1), dtype=torch.bfloat16) for i in range(200)]
    for t in dead:
        ops._fp8_derived(t)
    del dead, t
    assert len(ops._fp8_derived_cache) == 4200, "entries of live copies were dropped"
    ops._fp8_derived(torch.ones(3, 8, dtype=torch.bfloat16))  # a new entry above the limit: the dead ones go
    assert len(ops._fp8_derived_cache) <= 4001
    assert all(v[2]() is not None for key, v in ops._fp8_derived_cache.items() if key[1] != (3, 8))
    n = k.quants
    again = [ops._fp8_derived(t) for t in live]
    assert k.quants == n, "live entries must keep their (already current) copies"
    assert all(a is b for a, b in zip(again, first)), "live entries must keep their buffers"
