"""Generate tests/golden/adamw_master.pt from the UNMODIFIED reference, run on CPU through oracle/ref_shim.py.

    python tests/golden/make_adamw_master_golden.py        # needs the reference checkout ref_shim points at

The reference's optimiser leg in its `bf16: true`, `memory_efficient_bf16: false` arrangement (trainer.py:297-307 -> FP16Optimizer,
one_peace/optim/fp16_optimizer.py:13-250) on the micro model of make_golden.py's optim_fixture: three steps with layer-wise lr decay
groups and global-norm clipping.  What FP16Optimizer does around the wrapped optimiser is done here on a list of fp32 copies (its
`flatten=False` form; the arithmetic is element-wise, the norm global, so the flat form computes the same):

  build_fp32_params           fp32 copies of the bf16 parameters (a model `.float()` of the bf16 model, so that the reference's
                              get_parameter_groups names and groups them)
  _sync_fp16_grads_to_fp32    the bf16 gradients (oracle/synth.py: optim_grad) cast to fp32
  clip_grad_norm              fairseq's clip_grad_norm_(params, 0) for the norm, clip_coef = (max_norm / (norm + 1e-6)).clamp_(max=1)
  _unscale_grads              the fp32 gradients multiplied by that coefficient
  step                        the reference's Adam (optim/adam.py:124-253) over the fp32 copies
  _sync_fp32_params_to_fp16   the bf16 cast of every master

Stored: tensors and plain numbers only -- per step the gradient norm and, per parameter, the norm of its master, the master itself
(fp32) and its bf16 cast when it has at most FULL elements, else their first HEAD elements."""
import copy
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402
from oracle import synth  # noqa: E402
from tests.golden.make_golden import MICRO, OPTIM, build_ref_model  # noqa: E402

FULL, HEAD = 512, 128


def adamw_master_fixture():
    ro = R.ref_optim()
    m16, shapes = build_ref_model(MICRO, 1000)
    m16 = m16.to(torch.bfloat16)
    m32 = copy.deepcopy(m16).float()  # build_fp32_params: every master starts as the fp32 value of its bf16 parameter
    L = MICRO["layers"]
    assigner = ro.LayerDecayValueAssigner([OPTIM["layer_decay"] ** (L + 1 - i) for i in range(L + 2)])
    groups = ro.get_parameter_groups(m32, OPTIM["weight_decay"], m32.no_weight_decay(), assigner.get_layer_id, assigner.get_scale)
    opt = ro.Adam(groups, lr=OPTIM["lr"][0], betas=OPTIM["betas"], eps=OPTIM["eps"], weight_decay=OPTIM["weight_decay"])
    names = {id(p): n for n, p in m32.named_parameters()}
    assign = {}
    for gr in opt.param_groups:
        for p in gr["params"]:
            assert p.dtype == torch.float32
            assign[names[id(p)]] = (float(gr["lr_scale"]), float(gr["weight_decay"]))
    after, norms, coefs = [], [], []
    for step, lr in enumerate(OPTIM["lr"], start=1):
        for gr in opt.param_groups:  # optim/base_optimizer.py:8-14
            gr["lr"] = lr * gr["lr_scale"]
        for n, p in m32.named_parameters():  # _sync_fp16_grads_to_fp32
            p.grad = synth.optim_grad(n, p.shape, step).float()
        params = list(m32.parameters())
        norm = ro.clip_grad_norm_(params, 0)  # fp16_optimizer.py:192: the norm alone
        coef = (float(OPTIM["clip_norm"]) / (norm + 1e-6)).clamp_(max=1)  # :203
        for p in params:  # _unscale_grads -> multiply_grads
            p.grad.data.mul_(coef)
        opt.step()
        with torch.no_grad():  # _sync_fp32_params_to_fp16
            for p16, p32 in zip(m16.parameters(), m32.parameters()):
                p16.data.copy_(p32.data)
        norms.append(norm.float().clone())
        coefs.append(float(coef))
        snap = {}
        for (n, p32), p16 in zip(m32.named_parameters(), m16.parameters()):
            d32, d16 = p32.detach().reshape(-1), p16.detach().reshape(-1)
            snap[n + "#norm"] = d32.double().norm().float()
            k = d32.numel() if d32.numel() <= FULL else HEAD
            snap[n + "#master"] = d32[:k].clone()
            snap[n + "#bf16"] = d16[:k].clone()
        after.append(snap)
    fx = dict(cfg=MICRO, vocab=1000, shapes=shapes, optim=OPTIM, assign=assign, grad_norms=norms, clip_coefs=coefs, after=after)
    path = os.path.join(HERE, "adamw_master.pt")
    torch.save(fx, path)
    print("adamw_master: %d groups, grad norms %s, clip coefficients %s, %d bytes" % (
        len(opt.param_groups), [round(float(x), 4) for x in norms], [round(c, 4) for c in coefs], os.path.getsize(path)))


if __name__ == "__main__":
    adamw_master_fixture()
