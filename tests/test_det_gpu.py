"""OnePeaceDetViT in bf16 on the MI355X against tests/golden/det.pt, gated per tensor by the reference's OWN bf16 error on the CPU (both
sides of the gate come from the fixture), the standing gate of tests/test_video_gpu.py:

    rel_fro(HIP path, fp32 fixture)  <=  2.5 x rel_fro(reference in bf16, fp32 fixture)

with the shared table trained (the window kernel's dbias slabs carry its gradient) and frozen (no slabs asked for).  The window kernels
must actually have run, once each for the one window block (a spy on hip.attn_window_fwd / hip.attn_window_bwd).  The torch route of
the same bf16 model on the device is held to the same gate, and so is the difference between the two routes.  Every error goes to
det_parity_report.txt in the tests' output directory (tests/util.py: OUT)."""
import os

import pytest
import torch

from tests import det_util as D
from tests.util import OUT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 2.5
REPORT = os.path.join(OUT, "det_parity_report.txt")
TABLE = "image_adapter.rel_pos_table.weight"
_report_started = []
_runs = {}


class _Spy:
    NAMES = ("attn_window_fwd", "attn_window_bwd")

    def __init__(self):
        from one_peace_amd import hip
        self.hip, self.calls, self.kwargs = hip, [], []
        self.real = {n: getattr(hip, n) for n in self.NAMES}

    def _wrap(self, name):
        def f(*a, **k):
            self.calls.append(name)
            self.kwargs.append(k)
            return self.real[name](*a, **k)
        return f

    def __enter__(self):
        for n in self.NAMES:
            setattr(self.hip, n, self._wrap(n))
        return self

    def __exit__(self, *exc):
        for n in self.NAMES:
            setattr(self.hip, n, self.real[n])


def _run(route, table):
    """One bf16 forward + backward on the device per (route, table state), shared by the tests."""
    if (route, table) not in _runs:
        from one_peace_amd import ops
        fx = D.fixture()
        m = D.build(fx).to(DEV).to(torch.bfloat16)
        if table == "frozen":
            m.image_adapter.rel_pos_table.weight.requires_grad = False
        eligible = ops.hip_eligible
        if route == "torch":
            ops.hip_eligible = lambda x: False
        try:
            with _Spy() as spy:
                out, grads = D.run(m, fx, DEV, torch.bfloat16)
                torch.cuda.synchronize()
        finally:
            ops.hip_eligible = eligible
        _runs[(route, table)] = (out, grads, spy)
    return _runs[(route, table)]


def _write(lines):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a" if _report_started else "w") as f:   # one report per session
        _report_started.append(True)
        for line in lines:
            print(line)
            f.write(line + "\n")


@pytest.mark.parametrize("table", ["trained", "frozen"])
@pytest.mark.parametrize("route", ["fused", "torch"])
def test_bf16_model_is_within_the_references_own_bf16_error(route, table):
    fx = D.fixture()
    out, grads, spy = _run(route, table)
    if route == "fused":
        assert spy.calls == ["attn_window_fwd", "attn_window_bwd"], spy.calls          # one window block
        assert spy.kwargs[1]["want_dbias"] == (table == "trained") and spy.kwargs[1]["want_drel"] is True
    else:
        assert spy.calls == []
    names = [n for n in fx["grad_names"] if not (table == "frozen" and n == TABLE)]
    assert TABLE in fx["grad_names"] and (TABLE in grads) == (table == "trained")
    rows = [("output", D.rel_fro(out, fx["output"]), fx["ref_bf16_relerr"]["output"])]
    rows += [(n, D.rel_fro(grads[n], fx["grads"][n]), fx["ref_bf16_relerr"][n]) for n in names]
    _write(["%-5s %-8s %-44s hip %.3e  reference bf16 %.3e  ratio %.2f" % (route, table, what, mine, theirs, mine / theirs)
            for what, mine, theirs in rows])
    fails = [(what, mine, theirs) for what, mine, theirs in rows if not mine <= MARGIN * theirs]
    assert len(rows) >= 11 and not fails, fails


@pytest.mark.parametrize("table", ["trained", "frozen"])
def test_fused_and_torch_routes_agree_under_the_same_gate(table):
    fx = D.fixture()
    (fo, fg, _), (to, tg, _) = _run("fused", table), _run("torch", table)
    names = [n for n in fx["grad_names"] if not (table == "frozen" and n == TABLE)]
    rows = [("output", D.rel_fro(fo, to.float()), fx["ref_bf16_relerr"]["output"])]
    rows += [(n, D.rel_fro(fg[n], tg[n].float()), fx["ref_bf16_relerr"][n]) for n in names]
    _write(["f-t   %-8s %-44s diff %.3e reference bf16 %.3e  ratio %.2f" % (table, what, mine, theirs, mine / theirs)
            for what, mine, theirs in rows])
    fails = [(what, mine, theirs) for what, mine, theirs in rows if not mine <= MARGIN * theirs]
    assert not fails, fails


def _wide(**extra):
    """A model of the fixture's shape at twice the width (two heads): the width at which every row-wise op of the layer is a HIP op."""
    from one_peace_amd.one_peace_vision import OnePeaceDetViT
    torch.manual_seed(5)
    m = OnePeaceDetViT(**dict(D.fixture()["args"], embed_dim=128, ffn_embed_dim=128, attention_heads=2, **extra))
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "rel_pos" in n:
                p.copy_(0.02 * torch.randn(p.shape))
    return m.to(DEV).to(torch.bfloat16)


def test_fully_fused_layers_agree_with_the_torch_route():
    """embed_dim 128: ops.layer_norm, ops.packed_qkv, ops.linear and ops.ffn_branch around the window kernels.  There is no reference
    run of this model; the two routes of the SAME bf16 model are held to 2.5 x the largest error the reference's own bf16 run shows in
    the fixture for a tensor of that kind (output, resp. gradients)."""
    from one_peace_amd import ops
    fx = D.fixture()
    m = _wide().eval()
    x = D.image(fx).to(DEV, torch.bfloat16)
    cot = torch.randn(1, 128, 32, 32, device=DEV, dtype=torch.bfloat16)
    res = {}
    for route in ("fused", "torch"):
        eligible = ops.hip_eligible
        if route == "torch":
            ops.hip_eligible = lambda t: False
        try:
            m.zero_grad(set_to_none=True)
            with _Spy() as spy:
                out = m(x)["last_feat"]
                (out * cot).sum().backward()
                torch.cuda.synchronize()
        finally:
            ops.hip_eligible = eligible
        assert spy.calls == (["attn_window_fwd", "attn_window_bwd"] if route == "fused" else [])
        res[route] = (out.detach(), {n: p.grad.clone() for n, p in m.named_parameters()})
    assert all(layer.fused_supported(x) for layer in m.encoder.layers)
    gate_out = MARGIN * fx["ref_bf16_relerr"]["output"]
    gate_grad = MARGIN * max(v for k, v in fx["ref_bf16_relerr"].items() if k != "output")
    rows = [("output", D.rel_fro(res["fused"][0], res["torch"][0].float()), gate_out)]
    rows += [(n, D.rel_fro(g, res["torch"][1][n].float()), gate_grad) for n, g in res["fused"][1].items()]
    _write(["wide  f-t      %-44s diff %.3e gate %.3e" % r for r in rows])
    assert not [r for r in rows if not r[1] <= r[2]], [r for r in rows if not r[1] <= r[2]]


def test_training_step_with_stochastic_depth_and_checkpointing():
    fx = D.fixture()
    m = _wide(drop_path_rate=0.2, use_checkpoint=True).train()
    torch.manual_seed(0)
    with _Spy() as spy:
        out = m(D.image(fx).to(DEV, torch.bfloat16))["last_feat"]
        out.float().square().mean().backward()
        torch.cuda.synchronize()
    assert spy.calls == ["attn_window_fwd", "attn_window_fwd", "attn_window_bwd"], spy.calls    # the checkpoint's second forward
    for n, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad.float()).all()), n
