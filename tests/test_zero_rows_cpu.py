"""ops.SKIP_ZERO_ROWS on the host, without a GPU: which buffers leave the fill lists, when the row kernels get no multipliers (a null
predicate), and which entry point a wrapper calls.  The launches themselves are stubbed, as in tests/test_fwd_windows_cpu.py."""
import os

import pytest
import torch

BF = torch.bfloat16


def _segs(S=(64, 257, 250), B=(8, 6, 6), none=False):
    out, row0 = [], 0
    for s, b in zip(S, B):
        out.append((None if none else torch.ones(b), row0, s, b, 1))
        row0 += s * b
    return out, row0


def test_the_switch_comes_from_the_environment_and_defaults_to_on():
    from one_peace_amd import ops
    assert ops.SKIP_ZERO_ROWS == (os.environ.get("ONEPEACE_SKIP_ZERO_ROWS", "1") != "0")


@pytest.fixture
def recorded(monkeypatch):
    """ops._dgrad_windows with the launch stubbed: the outputs hip.live_mwindows was asked to fill, per call."""
    from one_peace_amd import hip, ops
    calls = []

    def live(segs, lists, outs):
        calls.append(list(outs))
        return [("list", "count")] * len(lists)
    monkeypatch.setattr(hip, "live_mwindows", live)
    monkeypatch.setattr(ops, "_dense_dgrad_sums_k_in_one_piece", lambda M, N, K, device: True)
    monkeypatch.setattr(ops, "SKIP_ZERO_DGRAD", True)
    return calls


def test_which_outputs_leave_the_backward_fill(recorded, monkeypatch):
    from one_peace_amd import ops
    segs, total = _segs()
    lists = [[(i, 0, 0) for i in range(3)]]
    dense = [(total, 256, 512)]
    a, b, c = (torch.empty(total, 256, dtype=BF) for _ in range(3))
    monkeypatch.setattr(ops, "SKIP_ZERO_ROWS", True)
    assert ops._dgrad_windows(segs, lists, [a], dense, unread=[b, c]) is not None
    assert [[id(o) for o in outs] for outs in recorded] == [[id(a)]]          # only what a dense reader needs is filled
    assert ops._dgrad_windows(segs, lists, [], dense, unread=[b, c]) is not None
    assert recorded[-1] == []                                                # every reader skips: the launch only builds lists
    assert ops._dgrad_windows(segs, lists, [a, b], dense) is not None
    assert [id(o) for o in recorded[-1]] == [id(a), id(b)]                    # (callers that name no unread output: as before)
    monkeypatch.setattr(ops, "SKIP_ZERO_ROWS", False)                         # ONEPEACE_SKIP_ZERO_ROWS=0: every output is filled, as before
    assert ops._dgrad_windows(segs, lists, [a], dense, unread=[b, c]) is not None
    assert [id(o) for o in recorded[-1]] == [id(a), id(b), id(c)]


def test_which_outputs_a_branch_names_as_unread():
    """ops._bwd_fills: the fill lists of the two backwards.  An output leaves the fill only where its ONLY reader takes the
    multipliers: d subLN(attn) and d LN_F(g) not without their LayerNorm (a dense kernel reads them then), d LN2(x) only in a
    one-segment branch; an output that is not computed (None) is in neither list."""
    from one_peace_amd import ops
    a, b = torch.empty(4, 8), torch.empty(4, 8)
    ids = lambda pair: tuple([id(o) for o in part] for part in pair)  # noqa: E731
    assert ids(ops._bwd_fills([(a, True), (b, True)])) == ([], [id(a), id(b)])      # attention branch with sub-LayerNorm; one-segment FFN
    assert ids(ops._bwd_fills([(a, False), (b, True)])) == ([id(a)], [id(b)])       # no sub-LayerNorm: attention reads d_aln
    assert ids(ops._bwd_fills([(a, True), (b, False)])) == ([id(b)], [id(a)])       # multi-modality FFN: LN2's backward stays dense
    assert ids(ops._bwd_fills([(a, False), (b, False)])) == ([id(a), id(b)], [])    # no LN_F, several segments: today's fill
    assert ids(ops._bwd_fills([(a, True), (None, True)])) == ([], [id(a)])          # d LN(x) not wanted


def test_no_lists_no_predicate(recorded, monkeypatch):
    """The callers pass the multipliers to a row kernel only when _dgrad_windows returned lists (zr_b = SKIP_ZERO_ROWS and lists): where
    the lists do not apply nothing is launched, every buffer keeps its dense writer and the predicate stays null."""
    from one_peace_amd import ops
    segs, total = _segs()
    lists = [[(i, 0, 0) for i in range(3)]]
    good = [(total, 256, 512)]
    b = torch.empty(total, 256, dtype=BF)
    monkeypatch.setattr(ops, "SKIP_ZERO_ROWS", True)
    assert ops._dgrad_windows(_segs(none=True)[0], lists, [], good, unread=[b]) is None      # no multipliers (layer 0, eval)
    assert ops._dgrad_windows(segs, lists, [], [(total, 256 + 128, 512)], unread=[b]) is None  # N % 256
    assert ops._dgrad_windows(segs, lists, [], [(total, 256, 96)], unread=[b]) is None         # K % 64, K < 128
    assert ops._dgrad_windows(segs, lists, [], good, unread=[torch.empty(total, 256)]) is None  # not bf16: checked for unread outputs too
    assert ops._dgrad_windows(segs, lists, [b] * 3, good, unread=[b] * 2) is None              # more than four outputs in all
    monkeypatch.setattr(ops, "_dense_dgrad_sums_k_in_one_piece", lambda M, N, K, device: False)
    assert ops._dgrad_windows(segs, lists, [], good, unread=[b]) is None                      # the dense launch would split K
    monkeypatch.setattr(ops, "_dense_dgrad_sums_k_in_one_piece", lambda M, N, K, device: True)
    monkeypatch.setattr(ops, "SKIP_ZERO_DGRAD", False)                                         # independent switches: no lists, no predicate
    assert ops._dgrad_windows(segs, lists, [], good, unread=[b]) is None
    assert recorded == []


def test_the_forward_fill_takes_an_output_that_needs_none(monkeypatch):
    """hip.live_mwindows_fwd: a None entry of outs (h0 | h1 under SKIP_ZERO_ROWS) never reaches the launch; its source goes with it."""
    from one_peace_amd import hip
    seen = []
    monkeypatch.setattr(hip, "_live_mwindows", lambda segs, lists, outs, srcs: seen.append((outs, srcs)) or ["win"])
    hh, out, x2 = (torch.empty(8, 16, dtype=BF) for _ in range(3))
    assert hip.live_mwindows_fwd("segs", "lists", [None, out], [None, x2]) == ["win"]
    assert len(seen[-1][0]) == 1 and seen[-1][0][0] is out and seen[-1][1][0] is x2
    hip.live_mwindows_fwd("segs", "lists", [hh, out], [None, x2])
    assert [o is t for o, t in zip(seen[-1][0], (hh, out))] == [True, True] and seen[-1][1][0] is None and seen[-1][1][1] is x2
    with pytest.raises(AssertionError):
        hip.live_mwindows_fwd("segs", "lists", [None], [None])


class _FakeLib:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 1 << 20 if name.endswith("workspace_bytes") else 0
        return fn


@pytest.fixture
def fake(monkeypatch):
    from one_peace_amd import hip
    lib = _FakeLib()
    monkeypatch.setattr(hip, "lib", lambda: lib)
    monkeypatch.setattr(hip, "stream", lambda: None)
    monkeypatch.setattr(hip, "workspace", lambda nbytes, device, tag="ws": torch.empty(16, dtype=torch.uint8))
    return lib


def test_a_wrapper_calls_the_new_entry_only_with_multipliers(fake):
    from one_peace_amd import hip
    rows, cols, S = 12, 16, 3
    h = torch.zeros(rows, 2 * cols, dtype=BF)
    w = torch.ones(cols, dtype=BF)
    st = torch.zeros(rows)
    ps = torch.ones(rows // S)
    hip.ln_geglu_fwd(h[:, :cols], h[:, cols:], w, w)
    hip.ln_geglu_fwd(h[:, :cols], h[:, cols:], w, w, ps=ps, rows_per_sample=S)
    hip.ln_geglu_bwd(h[:, :cols], h[:, :cols], h[:, cols:], w, st, st, need_wgrad=False)
    hip.ln_geglu_bwd(h[:, :cols], h[:, :cols], h[:, cols:], w, st, st, need_wgrad=False, ps=ps, rows_per_sample=S)
    x = torch.zeros(rows, cols, dtype=BF)
    hip.layernorm_bwd(x, x, w, w, st, st, need_wgrad=False)
    hip.layernorm_bwd(x, x, w, w, st, st, need_wgrad=False, ps=torch.ones(rows), rows_per_sample=1)
    hip.resid_bwd(x, rowscale=ps, rows_per_sample=S)
    hip.resid_bwd(x, rowscale=ps, rows_per_sample=S, skip_zero_rows=True)
    hip.resid_bwd(x, skip_zero_rows=True)                                     # no multipliers: the plain entry
    names = [n for n, _ in fake.calls if not n.endswith("workspace_bytes")]
    assert names == ["op_ln_geglu_fwd", "op_ln_geglu_fwd_skip", "op_ln_geglu_bwd", "op_ln_geglu_bwd_skip", "op_layernorm_bwd",
                     "op_layernorm_bwd_skip", "op_resid_bwd", "op_resid_bwd_skip", "op_resid_bwd"]
    by = dict((n, a) for n, a in fake.calls)
    assert by["op_ln_geglu_fwd_skip"][-3].value == ps.data_ptr() and by["op_ln_geglu_fwd_skip"][-2] == S
    assert by["op_ln_geglu_bwd_skip"][-3].value == ps.data_ptr() and by["op_ln_geglu_bwd_skip"][-2] == S
    assert by["op_layernorm_bwd_skip"][-2] == 1
    # fewer multipliers than samples, another dtype, the fp8 copy or a row table together with ps: refused on the host
    with pytest.raises(AssertionError):
        hip.ln_geglu_fwd(h[:, :cols], h[:, cols:], w, w, ps=ps[:3], rows_per_sample=S)
    with pytest.raises(AssertionError):
        hip.ln_geglu_bwd(h[:, :cols], h[:, :cols], h[:, cols:], w, st, st, need_wgrad=False, ps=ps.double(), rows_per_sample=S)
    with pytest.raises(AssertionError):
        hip.layernorm_bwd(x, x, w, w, st, st, need_wgrad=False, dx=x.clone(), x_rows=torch.zeros(rows, dtype=torch.int32), ps=ps, rows_per_sample=S)
    with pytest.raises(AssertionError):
        hip.ln_geglu_fwd(h[:, :cols], h[:, cols:], w, w, q8=(torch.zeros(rows, cols, dtype=torch.uint8), st), ps=ps, rows_per_sample=S)
