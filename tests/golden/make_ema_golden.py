"""Generate tests/golden/ema.pt from the UNMODIFIED reference, run on CPU.

    python tests/golden/make_ema_golden.py        # needs the reference checkout ref_shim points at

The reference's EMA (one_peace/utils/ema_module.py, loaded by file path: it needs only torch) with `ema_fp32: true`, decay 0.999 and
`ema_start_update: 2`, stepped as trainer.py:895-900 steps it -- after every update, with the new update count -- on the micro model of
make_golden.py over the three parameter states of adamw_master.pt's steps (the optimiser leg of make_adamw_master_golden.py, run
again here: the bf16 model after `_sync_fp32_params_to_fp16` is what the EMA reads).

Two runs:

  averaging   the model is handed over behind a wrapper whose `state_dict()` keeps `requires_grad` (`keep_vars=True`), so that
              `_step_internal` takes its averaging branch (:142-144).  Step 1 (updates 1 < ema_start_update) is a copy.
  as called   the model itself, as the trainer passes it: `state_dict()` detaches, `not param.requires_grad` (:139) holds for every key
              and every parameter is copied.  Stored as evidence that the class as called does not average.

Stored: tensors and plain numbers only -- per step and parameter the norm of the fp32 EMA and, for parameters of at most FULL elements
in full, else their first HEAD elements: the fp32 EMA (`#ema`) and the bf16 EMA model's value (`#bf16`); after the last step also the
fp32 "EMA" of the run as called (`#as_called`).  The bf16 parameters each step read are adamw_master.pt's `#bf16` entries of the same
step and cut (checked here against that file), so they are not stored again."""
import copy
import importlib.util
import os
import sys
from types import SimpleNamespace

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402
from oracle import synth  # noqa: E402
from tests.golden.make_adamw_master_golden import FULL, HEAD  # noqa: E402
from tests.golden.make_golden import MICRO, OPTIM, build_ref_model  # noqa: E402

EMA = dict(decay=0.999, start_update=2)


class KeepVars:
    """What EMAModule.step reads of a model, with `state_dict()` keeping the parameters' `requires_grad`."""

    def __init__(self, model):
        self.model = model

    def state_dict(self):
        return self.model.state_dict(keep_vars=True)

    def named_buffers(self):
        return self.model.named_buffers()


def ema_fixture():
    spec = importlib.util.spec_from_file_location("_ref_ema_module", os.path.join(R.REFERENCE_ROOT, "one_peace", "utils", "ema_module.py"))
    ref_ema = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref_ema)
    ro = R.ref_optim()
    m16, shapes = build_ref_model(MICRO, 1000)
    m16 = m16.to(torch.bfloat16)
    m32 = copy.deepcopy(m16).float()
    L = MICRO["layers"]
    assigner = ro.LayerDecayValueAssigner([OPTIM["layer_decay"] ** (L + 1 - i) for i in range(L + 2)])
    groups = ro.get_parameter_groups(m32, OPTIM["weight_decay"], m32.no_weight_decay(), assigner.get_layer_id, assigner.get_scale)
    opt = ro.Adam(groups, lr=OPTIM["lr"][0], betas=OPTIM["betas"], eps=OPTIM["eps"], weight_decay=OPTIM["weight_decay"])
    cfg = SimpleNamespace(ema_decay=EMA["decay"], ema_fp32=True, ema_start_update=EMA["start_update"])
    averaging, as_called = ref_ema.EMAModule(m16, cfg), ref_ema.EMAModule(m16, cfg)
    states = torch.load(os.path.join(HERE, "adamw_master.pt"), weights_only=True)["after"]
    after, decays = [], []
    for step, lr in enumerate(OPTIM["lr"], start=1):  # make_adamw_master_golden.py: the FP16Optimizer leg
        for gr in opt.param_groups:
            gr["lr"] = lr * gr["lr_scale"]
        for n, p in m32.named_parameters():
            p.grad = synth.optim_grad(n, p.shape, step).float()
        params = list(m32.parameters())
        norm = ro.clip_grad_norm_(params, 0)
        coef = (float(OPTIM["clip_norm"]) / (norm + 1e-6)).clamp_(max=1)
        for p in params:
            p.grad.data.mul_(coef)
        opt.step()
        with torch.no_grad():
            for p16, p32 in zip(m16.parameters(), m32.parameters()):
                p16.data.copy_(p32.data)
        averaging.step(KeepVars(m16), step)  # trainer.py:897-900
        as_called.step(m16, step)
        decays.append(float(averaging.get_decay()))
        ema_model = averaging.get_model().state_dict()
        snap = {}
        for n, p16 in m16.named_parameters():
            e32 = averaging.fp32_params[n].detach().reshape(-1)
            assert e32.dtype == torch.float32 and ema_model[n].dtype == torch.bfloat16
            k = e32.numel() if e32.numel() <= FULL else HEAD
            snap[n + "#norm"] = e32.double().norm().float()
            snap[n + "#ema"] = e32[:k].clone()
            snap[n + "#bf16"] = ema_model[n].detach().reshape(-1)[:k].clone()
            assert torch.equal(p16.detach().reshape(-1)[:k].view(torch.int16), states[step - 1][n + "#bf16"].view(torch.int16)), (step, n)
            if step == len(OPTIM["lr"]):
                snap[n + "#as_called"] = as_called.fp32_params[n].detach().reshape(-1)[:k].clone()
        after.append(snap)
    fx = dict(cfg=MICRO, vocab=1000, shapes=shapes, optim=OPTIM, ema=EMA, decays=decays, after=after)
    path = os.path.join(HERE, "ema.pt")
    torch.save(fx, path)
    last = after[-1]
    moved = sum(int((last[k] != states[-1][k[:-4] + "#bf16"].float()).sum()) for k in last if k.endswith("#ema"))
    copied = sum(int((last[k] != states[-1][k[:-10] + "#bf16"].float()).sum()) for k in last if k.endswith("#as_called"))
    print("ema: decays %s, %d stored elements of the averaging run differ from the last parameters, %d of the run as called; %d bytes" % (
        decays, moved, copied, os.path.getsize(path)))


if __name__ == "__main__":
    ema_fixture()
