"""The fp32 weight average without a GPU: the criterion of tests/ema_ref.py against planted faults; ema.FlatEMA.step() and
optim.TorchAdamW(ema=) against the reference's EMAModule (tests/golden/ema.pt), bit for bit; the stored evidence that the reference class as
its trainer calls it copies instead of averaging; the checkpoint surface, applied() and reverse(); the refusals; a 100-step run of tiny
updates that an fp32 average follows and a bf16 one does not; fp32 parameters (the average owns its storage); the ABI entries."""
import ctypes
import os
import re

import pytest
import torch

from tests import adamw_master_ref as M
from tests import adamw_ref as R
from tests import ema_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------
# the criterion against planted faults
# ------------------------------------------------------------------------------------------------------------------
_PLANT = {}


def _plant_state():
    """One AdamW step (step 1, lr 1e-2, the bf16-only arrangement) in the fp32 emulation of adamw_master_ref: the unrounded fp32 result,
    its bf16 cast (what is stored), the old parameter and a lagging average.  Computed once."""
    if not _PLANT:
        n = 1 << 16
        _, p, g, m, v, e = E.make_ema_state(n, 1, seed=21)
        lr, b1, b2, eps, wd0 = R.HYPER[0]
        new, pb, _, _ = M.emulate_master_fp32(p.float(), p, g, m, v, 1, lr, b1, b2, eps, weight_decay=wd0)
        assert E.changed_share(pb, p) >= 0.99
        _PLANT.update(p_old=p, new=new, p_hat=pb, e=e)
    return _PLANT


@pytest.mark.parametrize("decay", [0.9999, 0.999, 0.99, 0.5, 0.0])
def test_the_clean_emulation_passes_the_criterion(decay):
    s = _plant_state()
    keep, take = E.coefficients(decay)
    got = E.emulate_ema_fp32(s["e"], s["p_old"], s["new"], decay)
    E.assert_step(got, s["e"], s["p_hat"], keep, take, "clean %g" % decay)
    if decay == 0.0:
        assert torch.equal(got, s["p_hat"].float())


# the unrounded fp32 parameter differs from the stored one by at most half a bf16 spacing, 2^-9 |p|; times take = 1e-4 that is below the
# bound 2^-24 (...) ~ 2^-23 |e|: at 0.9999 the criterion cannot see this fault, and is not asked to
PLANT_CASES = [(d, f) for d in (0.9999, 0.99) for f in E.PLANTED if not (f == "unrounded_parameter" and d == 0.9999)]


@pytest.mark.parametrize("decay,planted", PLANT_CASES)
def test_a_planted_fault_fails_the_criterion_on_99_percent_of_the_elements(decay, planted):
    s = _plant_state()
    keep, take = E.coefficients(decay)
    got = E.emulate_ema_fp32(s["e"], s["p_old"], s["new"], decay, planted)
    apart = E.apart(got, s["e"], s["p_hat"], keep, take)
    rejected = E.rejected(got, s["e"], s["p_hat"], keep, take)
    print("%s at %g: %.4f more than twice the bound apart, %.4f rejected" % (planted, decay, apart, rejected))
    assert apart >= 0.99, "the state does not show the fault: only %.4f of the elements are twice the bound apart" % apart
    assert rejected >= 0.99, (planted, decay, rejected)


# ------------------------------------------------------------------------------------------------------------------
# the reference's arithmetic
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixtures(golden_dir):
    return (torch.load(os.path.join(golden_dir, "adamw_master.pt"), weights_only=False),
            torch.load(os.path.join(golden_dir, "ema.pt"), weights_only=False))


def test_flat_ema_step_reproduces_the_reference_bit_for_bit(fixtures):
    """FlatEMA.step() on the CPU, fed the reference's bf16 parameters of every step on the stored elements: the fp32 average, the bf16
    EMA model (ema_state) and, for parameters stored in full, the norm -- as the reference left them.  Step 1 is the copy."""
    from one_peace_amd.ema import FlatEMA
    fx, fe = fixtures
    model, flat = E.fixture_model(fx, "cpu")
    ema = FlatEMA(flat, decay=fe["ema"]["decay"], start_update=fe["ema"]["start_update"])
    assert ema.num_updates == 0 and torch.equal(ema.shadow, flat.params.float())
    for step in (1, 2, 3):
        states, want = fx["after"][step - 1], fe["after"][step - 1]
        with torch.no_grad():
            for n, _, o, _ in flat.entries:
                ref_p = states[n + "#bf16"]
                flat.params[o:o + ref_p.numel()].copy_(ref_p)
        ema.step(step)
        assert ema.num_updates == step and ema.decay_at(step) == fe["decays"][step - 1]
        if step == 1:
            assert torch.equal(ema.shadow, flat.params.float())
        state = ema.ema_state(model)
        for n, p, o, k in flat.entries:
            ref_e = want[n + "#ema"]
            j = ref_e.numel()
            assert torch.equal(ema.shadow[o:o + j].view(torch.int32), ref_e.view(torch.int32)), (step, n)
            assert state[n].dtype == torch.bfloat16 and state[n].shape == p.shape
            assert torch.equal(M.bits16(state[n].reshape(-1)[:j]), M.bits16(want[n + "#bf16"])), (step, n)
            if j == k:
                assert float(ema.shadow[o:o + k].double().norm().float()) == float(want[n + "#norm"]), (step, n)
    stored = [(o, fe["after"][-1][n + "#ema"].numel()) for n, _, o, _ in flat.entries]
    moved = sum(int((ema.shadow[o:o + j] != flat.params[o:o + j].float()).sum()) for o, j in stored)
    assert moved > 0.4 * sum(j for _, j in stored)  # the average is not the weights


def test_torch_adamw_with_ema_reproduces_the_reference_bit_for_bit(fixtures):
    from one_peace_amd.optim import TorchAdamW
    worst, worst_ref, unlike_bits, compared = E.run_golden(fixtures[0], fixtures[1], TorchAdamW, "cpu")
    assert unlike_bits == 0 and worst <= 1.0 and worst_ref <= 1.0 and compared > 20000


def test_the_reference_class_as_its_trainer_calls_it_copies(fixtures):
    """Documents the reference: one_peace/utils/ema_module.py walks state_dict(), whose tensors are detached, so every parameter takes
    the copy branch -- after three steps at decay 0.999 its fp32 "EMA" IS the last weights, while the averaging run's is not."""
    fx, fe = fixtures
    last, params = fe["after"][-1], fx["after"][-1]
    keys = [k[:-len("#as_called")] for k in last if k.endswith("#as_called")]
    assert len(keys) > 50
    differ = 0
    for n in keys:
        assert torch.equal(last[n + "#as_called"], params[n + "#bf16"].float()), n
        differ += int((last[n + "#ema"] != params[n + "#bf16"].float()).sum())
    assert differ > 10000


def test_the_fixture_holds_tensors_and_plain_numbers_only(golden_dir):
    path = os.path.join(golden_dir, "ema.pt")
    assert os.path.getsize(path) < 1000000
    fe = torch.load(path, weights_only=True)  # refuses anything but tensors, numbers, strings and plain containers
    assert len(fe["after"]) == 3 and fe["decays"] == [0.0, 0.999, 0.999] and fe["ema"] == {"decay": 0.999, "start_update": 2}
    assert all(t.dtype == (torch.bfloat16 if k.endswith("#bf16") else torch.float32) for snap in fe["after"] for k, t in snap.items())


# ------------------------------------------------------------------------------------------------------------------
# the surface
# ------------------------------------------------------------------------------------------------------------------
class Small(torch.nn.Module):
    """A matrix of 15 elements (padded to 16 in the flat buffer), a bias, a frozen parameter and a buffer."""

    def __init__(self, seed):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        self.lin = torch.nn.Linear(5, 3)
        self.frozen = torch.nn.Parameter(torch.randn(4, generator=gen), requires_grad=False)
        self.register_buffer("count", torch.arange(3.0))
        with torch.no_grad():
            self.lin.weight.copy_(torch.randn(3, 5, generator=gen))
            self.lin.bias.copy_(torch.randn(3, generator=gen))


def _small(seed, steps=3):
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.ema import FlatEMA
    model = Small(seed).to(torch.bfloat16)
    flat = FlatParameters(model)
    ema = FlatEMA(flat, decay=0.9)
    gen = torch.Generator().manual_seed(seed + 100)
    for _ in range(steps):
        with torch.no_grad():
            flat.params.add_((0.1 * torch.randn(flat.numel, generator=gen)).to(torch.bfloat16))
        ema.step()
    return model, flat, ema


def test_ema_state_fp32_params_and_restore_round_trip():
    model, flat, ema = _small(1)
    assert ema.num_updates == 3 and not torch.equal(ema.shadow, flat.params.float())
    state, fp32 = ema.ema_state(model), ema.fp32_params()
    assert list(state) == list(model.state_dict()) and set(fp32) == {"lin.weight", "lin.bias"}
    assert torch.equal(state["frozen"], model.frozen) and torch.equal(state["count"], model.count)
    for n, p, o, k in flat.entries:
        assert fp32[n].dtype == torch.float32 and fp32[n].shape == p.shape and fp32[n].data_ptr() == ema.shadow[o:o + k].data_ptr()
        assert state[n].dtype == torch.bfloat16 and torch.equal(state[n], fp32[n].to(torch.bfloat16))
        assert not torch.equal(state[n], p)
    # into another average, over another model: fp32 values when they are given ...
    _, flat2, ema2 = _small(2, steps=1)
    ema2.restore(dict(state, unknown=torch.zeros(2)), fp32)
    assert flat2.entries[0][2:] == flat.entries[0][2:]
    for _, _, o, k in flat2.entries:
        assert torch.equal(ema2.shadow[o:o + k].view(torch.int32), ema.shadow[o:o + k].view(torch.int32))
    # ... built from the bf16 state otherwise; a key missing from both is skipped
    _, flat3, ema3 = _small(3, steps=1)
    before = ema3.shadow.clone()
    ema3.restore({k: v for k, v in state.items() if k != "lin.bias"})
    for n, _, o, k in flat3.entries:
        want = before[o:o + k] if n == "lin.bias" else state[n].float().reshape(-1)
        assert torch.equal(ema3.shadow[o:o + k], want), n
    # fp32 values for one parameter only: the other comes from the state
    _, flat4, ema4 = _small(4, steps=1)
    ema4.restore(state, {"lin.weight": fp32["lin.weight"]})
    for n, _, o, k in flat4.entries:
        want = fp32[n].reshape(-1) if n == "lin.weight" else state[n].float().reshape(-1)
        assert torch.equal(ema4.shadow[o:o + k], want), n


def test_restore_raises_on_a_tensor_of_another_shape_before_it_writes_anything():
    model, flat, ema = _small(8)
    state, fp32 = ema.ema_state(model), ema.fp32_params()
    _, flat2, ema2 = _small(9, steps=1)
    before = ema2.shadow.clone()
    for bad in (dict(state, **{"lin.bias": torch.zeros(4, dtype=torch.bfloat16)}),      # another size
                dict(state, **{"lin.weight": state["lin.weight"].t().contiguous()})):  # the same size, transposed
        with pytest.raises(ValueError, match="shape"):
            ema2.restore(bad)
        with pytest.raises(ValueError, match="shape"):
            ema2.restore(state, {k: v for k, v in bad.items() if k.startswith("lin.")})
        assert torch.equal(ema2.shadow, before), "a refused restore wrote part of the average"


# ------------------------------------------------------------------------------------------------------------------
# fp32 parameters: the "anything else" route of step(), where .float() of the parameters would be the parameters themselves
# ------------------------------------------------------------------------------------------------------------------
def _bits32(t):
    return t.detach().contiguous().view(torch.int32)


def test_fp32_parameters_keep_an_average_of_their_own():
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.ema import FlatEMA
    model = Small(10)  # fp32
    flat = FlatParameters(model)
    assert flat.params.dtype == torch.float32
    ema = FlatEMA(flat, decay=0.9)
    assert ema.shadow.dtype == torch.float32 and ema.shadow.data_ptr() != flat.params.data_ptr()
    assert ema.shadow.untyped_storage().data_ptr() != flat.params.untyped_storage().data_ptr()
    keep, take = E.coefficients(0.9)
    gen = torch.Generator().manual_seed(110)
    for _ in range(3):
        with torch.no_grad():
            flat.params.add_(0.1 * torch.randn(flat.numel, generator=gen))
        p0, e0 = flat.params.clone(), ema.shadow.clone()
        ema.step()
        assert torch.equal(_bits32(flat.params), _bits32(p0)), "ema.step() wrote the parameters"
        # the criterion of ema_ref.py holds for any fp32 p^ (nothing in its derivation uses that p^ is a bf16 value)
        E.assert_step(ema.shadow, e0, p0, keep, take, "fp32 parameters")
    assert not torch.equal(ema.shadow, flat.params)
    state = ema.ema_state(model)
    assert state["lin.weight"].dtype == torch.float32 and state["lin.weight"].data_ptr() != ema.fp32_params()["lin.weight"].data_ptr()
    before, avg = flat.params.clone(), ema.shadow.clone()
    with ema.applied():
        assert torch.equal(_bits32(flat.params), _bits32(avg)) and torch.equal(_bits32(ema.shadow), _bits32(avg))
    assert torch.equal(_bits32(flat.params), _bits32(before)), "applied() did not restore the parameters"
    assert torch.equal(_bits32(ema.shadow), _bits32(avg)), "applied() lost the average"
    ema.reverse()
    assert torch.equal(_bits32(flat.params), _bits32(avg)) and ema.shadow.data_ptr() != flat.params.data_ptr()


def test_torch_adamw_with_ema_on_fp32_parameters_steps_the_weights_as_without_it():
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import TorchAdamW
    runs = {}
    for with_ema in (False, True):
        model = Small(11)
        flat = FlatParameters(model)
        ema = FlatEMA(flat, decay=0.99) if with_ema else None
        opt = TorchAdamW(flat, lr=1e-2, ema=ema)
        gen = torch.Generator().manual_seed(111)
        history = []
        for _ in range(4):
            flat.grads.copy_(torch.randn(flat.numel, generator=gen))
            opt.step()
            history.append(flat.params.clone())
        runs[with_ema] = (history, ema)
    for a, b in zip(runs[False][0], runs[True][0]):
        assert torch.equal(_bits32(a), _bits32(b)), "the average changed the training weights"
    ema = runs[True][1]
    keep, take = E.coefficients(0.99)
    model = Small(11)
    run = E.Fp64Run(FlatParameters(model).params)
    for p in runs[True][0]:
        run.step(p, keep, take)
    assert ema.num_updates == 4 and run.used(ema.shadow) <= 1.0
    assert not torch.equal(ema.shadow, runs[True][0][-1])


def test_applied_swaps_the_average_in_and_restores_the_parameters_bit_for_bit():
    model, flat, ema = _small(5)
    before = flat.params.clone()
    want = ema.shadow.to(torch.bfloat16)
    assert not torch.equal(M.bits16(want), M.bits16(before))
    with ema.applied() as inside:
        assert inside is ema
        assert torch.equal(M.bits16(flat.params), M.bits16(want))
        o = {n: o for n, _, o, _ in flat.entries}["lin.weight"]
        assert torch.equal(model.lin.weight.detach().reshape(-1), want[o:o + 15])  # the model's parameters are views of the buffer
    assert torch.equal(M.bits16(flat.params), M.bits16(before))
    with pytest.raises(KeyError):
        with ema.applied():
            assert torch.equal(M.bits16(flat.params), M.bits16(want))
            raise KeyError("the body raises")
    assert torch.equal(M.bits16(flat.params), M.bits16(before))
    assert torch.equal(ema.shadow.to(torch.bfloat16), want)  # the average itself is not touched


def test_reverse_writes_the_average_into_the_parameters():
    model, flat, ema = _small(6)
    want = ema.shadow.to(torch.bfloat16)
    ema.reverse()
    assert torch.equal(M.bits16(flat.params), M.bits16(want))
    assert all(torch.equal(p.detach().reshape(-1), want[o:o + k]) for _, p, o, k in flat.entries)


def test_step_counts_and_coefficients():
    from one_peace_amd.ema import FlatEMA
    _, flat, _ = _small(7, steps=0)
    ema = FlatEMA(flat, decay=0.9999, start_update=3)
    assert ema.coefficients(2) == (0.0, 1.0)
    keep, take = ema.coefficients(3)
    assert (keep, take) == (R.f32(0.9999), R.f32(1.0 - 0.9999)) and take != R.f32(1.0 - R.f32(0.9999))  # the subtraction in double
    ema.step()
    ema.step()
    assert ema.num_updates == 2 and torch.equal(ema.shadow, flat.params.float())
    ema.step(updates=10)
    assert ema.num_updates == 10
    ema.step()
    assert ema.num_updates == 11


# ------------------------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------------------------
def test_what_is_not_built_is_refused_with_a_reason():
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import FusedAdamW, TorchAdamW
    flat = FlatParameters(M.EightParams(1.0).to(torch.bfloat16))
    with pytest.raises(ValueError, match="bf16"):
        FlatEMA(flat, ema_fp32=False)
    with pytest.raises(ValueError, match="skip_keys"):
        FlatEMA(flat, skip_keys={"w"})
    ema = FlatEMA(flat)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedAdamW(flat, ema=ema)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        FusedAdamW(flat, master_weights=True, ema=ema)
    other = FlatParameters(M.EightParams(1.0).to(torch.bfloat16))
    with pytest.raises(ValueError, match="other FlatParameters"):
        TorchAdamW(other, ema=ema)


# ------------------------------------------------------------------------------------------------------------------
# 100 steps of tiny updates at the default decay
# ------------------------------------------------------------------------------------------------------------------
def test_hundred_tiny_updates_move_an_fp32_average_and_not_a_bf16_one():
    """adamw_master_ref's case "one" (1.0, lr 1e-4, with the master: the bf16 parameter walks down to 0.98828125) beside an average at
    decay 0.9999: the fp32 average stays within the summed per-step bound of the fp64 run; the same run with the average stored through
    bf16 after every step ends where it started -- take * (p - e) <= 1e-4 * 0.012 against half a bf16 spacing below 1, 2^-9."""
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import TorchAdamW
    start, lr, end_bf16 = M.HUNDRED["one"]
    model = M.EightParams(start).to(torch.bfloat16)
    flat = FlatParameters(model)
    ema = FlatEMA(flat, decay=0.9999)
    opt = TorchAdamW(flat, lr=lr, betas=M.HUNDRED_BETAS, eps=M.HUNDRED_EPS, weight_decay=0.0, master_weights=True, ema=ema)
    keep, take = E.coefficients(0.9999)
    run, e0 = E.Fp64Run(ema.shadow), ema.shadow.clone()
    in_bf16 = e0.to(torch.bfloat16)
    for _ in range(M.HUNDRED_STEPS):
        model.w.grad.fill_(M.HUNDRED_GRAD)
        opt.step()
        run.step(flat.params, keep, take)
        in_bf16 = (in_bf16.float() * torch.tensor(keep, dtype=torch.float32) + torch.tensor(take, dtype=torch.float32) * flat.params.float()).to(torch.bfloat16)
    assert ema.num_updates == M.HUNDRED_STEPS and bool((flat.params.double() == end_bf16).all())
    used = run.used(ema.shadow)
    print("100 steps: average %.9g (fp64 %.9g), %.3f of the summed bound" % (float(ema.shadow[0]), float(run.e[0]), used))
    assert used <= 1.0
    assert bool((ema.shadow < e0).all()) and float((e0 - ema.shadow).min()) > 3e-5  # sum_t 1e-4 (1 - p_t): it moved
    assert torch.equal(M.bits16(in_bf16), M.bits16(e0.to(torch.bfloat16))), "an average kept in bf16 was expected to stay where it started"


# ------------------------------------------------------------------------------------------------------------------
# ABI
# ------------------------------------------------------------------------------------------------------------------
def _header_args(name):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "onepeace_hip.h")).read(), flags=re.S)
    found = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert found, "%s is not declared in include/onepeace_hip.h" % name
    return [" ".join(a.split()) for a in found.group(1).split(",")]


def test_abi_entries_and_ctypes_arity():
    from one_peace_amd import hip
    assert _header_args("op_ema_step") == ["float* ema", "const void* p", "int64_t numel", "float keep", "float take", "void* stream"]
    res, argtypes = hip.SIGNATURES["op_ema_step"]
    assert res is ctypes.c_int and len(argtypes) == 6 and argtypes[3] is ctypes.c_float and argtypes[4] is ctypes.c_float
    args, old = _header_args("op_adamw_step_groups_ema"), _header_args("op_adamw_step_groups_master")
    assert len(args) == 22 and args[5] == "float* ema" and args[-3:-1] == ["float ema_keep", "float ema_take"]
    assert args[:5] + args[6:-3] + args[-1:] == old
    res, argtypes = hip.SIGNATURES["op_adamw_step_groups_ema"]
    _, old_types = hip.SIGNATURES["op_adamw_step_groups_master"]
    assert res is ctypes.c_int and argtypes[:5] + argtypes[6:-3] + argtypes[-1:] == old_types
    assert argtypes[5] is ctypes.c_void_p and argtypes[-3] is ctypes.c_float and argtypes[-2] is ctypes.c_float
    assert callable(hip.ema_step) and callable(hip.adamw_step_groups_ema)
    if os.path.exists(hip.LIB_PATH):
        L = ctypes.CDLL(hip.LIB_PATH)
        assert hasattr(L, "op_ema_step") and hasattr(L, "op_adamw_step_groups_ema")
        L.op_abi_version.restype = ctypes.c_int
        assert L.op_abi_version() == 10
