"""The masked-token (DCL) oracle against the torch branch of criterions/pretrain.py:compute_dcl_loss, without a GPU.

O.dcl_loss is written from the formula of image_text_pretrain_loss.py:187-208; the mirror's torch branch must compute the
same loss and the same student gradient, with and without padding masks and with label smoothing."""
import pytest
import torch

from oracle import onepeace_oracle as O


def dcl_inputs(B, L, H, seed, dtype, pad=False):
    g = torch.Generator().manual_seed(seed)
    student = torch.randn(B, L, H, generator=g).to(dtype)
    teacher = torch.randn(B, L, H, generator=g).to(dtype)
    mask = torch.rand(B, L, generator=g) < 0.4
    mask[:, 0] = False
    mask[0, 1] = True  # at least one masked token
    pads = None
    if pad:  # right padding of a different length per sample, over the non-CLS positions
        lens = torch.randint(2, L, (B,), generator=g)
        lens[0] = L - 1
        pads = torch.arange(L - 1)[None, :] >= lens[:, None]
    return student, teacher, mask, pads


@pytest.mark.parametrize("pad", [False, True])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_dcl_oracle_matches_torch_branch(pad, eps, dtype):
    from one_peace_amd.criterions.pretrain import compute_dcl_loss
    student, teacher, mask, pads = dcl_inputs(3, 11, 16, seed=7, dtype=dtype, pad=pad)
    s1, s2 = student.clone().requires_grad_(True), student.clone().requires_grad_(True)
    got = compute_dcl_loss(s1, teacher, mask, 2.5, eps, pads)
    ref = O.dcl_loss(s2, teacher, mask, 2.5, eps, pads)
    got.backward()
    ref.backward()
    # the two run the same torch ops in the same order, so loss and gradient are bit-identical
    assert torch.equal(got, ref)
    assert torch.equal(s1.grad, s2.grad)
    assert s1.grad[:, 0].abs().max() == 0  # CLS takes no part


def test_dcl_oracle_formula_fp64():
    """fp64: O.dcl_loss equals an explicit fp64 evaluation of the smoothed NLL over the kept tokens, and padding drops
    both the padded rows and the padded columns."""
    student, teacher, mask, pads = dcl_inputs(2, 9, 8, seed=3, dtype=torch.float64, pad=True)
    eps, scale = 0.1, 2.5
    ref = O.dcl_loss(student, teacher, mask, scale, eps, pads)
    keep = ~pads.reshape(-1)
    s = student[:, 1:].reshape(-1, 8)[keep]
    t = teacher[:, 1:].reshape(-1, 8)[keep]
    m = mask[:, 1:].reshape(-1)[keep]
    n = t.shape[0]
    s = s / s.norm(dim=1, keepdim=True)
    t = t / t.norm(dim=1, keepdim=True)
    losses = []
    for i in torch.nonzero(m).flatten().tolist():
        logits = scale * (t @ s[i])
        lp = logits - torch.logsumexp(logits, 0)
        e = eps / (n - 1)
        losses.append(-(1 - eps - e) * lp[i] - e * lp.sum())
    assert torch.allclose(ref, torch.stack(losses).mean(), rtol=1e-13, atol=0)
    assert ref.dtype == torch.float64
