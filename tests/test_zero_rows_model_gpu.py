"""A training step whose row kernels leave out the rows of dropped samples and whose fills no longer write them (ops.SKIP_ZERO_ROWS)
is the step with the dense row kernels and the full fills, bit for bit -- also when every buffer the step allocates starts out as
NaN, so that a row nobody wrote would show wherever a reader does not skip it."""
from types import SimpleNamespace

import pytest
import torch

from oracle import synth
from tests.model_util import TinyDictionary, load_synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
SWITCHES = ("SKIP_ZERO_ROWS", "SKIP_ZERO_FWD", "SKIP_ZERO_DGRAD", "SKIP_ZERO_BACKWARD")


def poison_allocator(rows, H, F):
    """NaN-filled bf16 and fp32 buffers of the step's activation sizes, allocated and freed: the caching allocator hands their memory
    to the step's torch.empty calls."""
    held = []
    for n in rows:
        for cols in (H, 3 * H, F, 2 * F):
            for _ in range(3):
                held.append(torch.full((n, cols), float("nan"), dtype=BF, device=DEV))
        for _ in range(8):
            held.append(torch.full((n,), float("nan"), dtype=torch.float32, device=DEV))
            held.append(torch.full((n, H), float("nan"), dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    del held


@pytest.mark.parametrize("cheap,lock_step", [(False, True), (True, True), (False, False)])
def test_training_step_is_bit_identical_with_and_without_the_row_skips(cheap, lock_step):
    """Lock-step tri-modal, 2 layers: text 64 rows (aligned tiles), image 257 (a window per kept sample + the strided last rows), audio
    250 (a window per kept sample); H = 256, the smallest the listed route takes; 64 samples per modality (below that gamma's gradient
    wants the branch output and no launch is listed: tests/test_fwd_windows_model_gpu.py).  Drop probability 0.5 with a seeded mask.
    Three legs per mode under the same mask: SKIP_ZERO_ROWS on, off, and all four zero-skipping switches off (every launch dense).
    lock_step False: one encoder pass per modality, so every branch has ONE segment with per-sample multipliers (rps = S): the
    LayerNorm backward of LN2 skips too and d LN2(x) leaves the fill, which the lock-step FFN branch (three segments) keeps."""
    from one_peace_amd import hip, ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from one_peace_amd.optim import FusedAdamW
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    H, F, B = 256, 512, 64
    cfg = dict(embed_dim=H, ffn_embed_dim=F, layers=2, attention_heads=4, image_rel_bucket_size=16, text_bucket_size=256,
               audio_bucket_size=512)
    assert synth.audio_frames(80000) + 1 == 250
    inp = synth.synth_inputs(B, text_len=63, image_res=256, audio_samples=80000, vocab=1000)
    inp = {k: (v.to(DEV).to(BF) if v.is_floating_point() else v.to(DEV)) for k, v in inp.items()}
    seg_rows = (64 * B, 257 * B, 250 * B)
    mask = torch.bernoulli(torch.full((2, 3 * B), 0.5), generator=torch.Generator(device="cpu").manual_seed(11)).bool()
    for branch in range(2):
        for m in range(3):
            part = mask[branch, m * B:(m + 1) * B]
            assert 0 < int(part.sum()) < B, "the mask must drop and keep a sample of every modality in every branch"

    passes = []

    def fixed_scales(self, nb, device):
        if lock_step:
            assert nb == 3 * B
            part = mask
        else:  # the k-th pass of a leg takes the k-th third of the mask: the same samples in every leg
            assert nb == B
            part = mask[:, (len(passes) % 3) * B:(len(passes) % 3 + 1) * B]
            passes.append(nb)
        return [(None, None), ((part[0].float() / 0.5).to(device), (part[1].float() / 0.5).to(device))]
    saved = {n: getattr(ops, n) for n in SWITCHES}
    orig_scales = TE.TransformerEncoder._draw_path_scales
    orig = {n: getattr(hip, n) for n in ("ln_geglu_fwd", "ln_geglu_bwd", "layernorm_bwd", "resid_bwd", "live_mwindows_fwd", "live_mwindows")}
    old_cheap = ops.set_recompute_cheap(cheap)
    res, used = {}, {}
    try:
        TE.TransformerEncoder._draw_path_scales = fixed_scales
        for leg, on in (("rows", dict(SKIP_ZERO_ROWS=True)), ("no_rows", dict(SKIP_ZERO_ROWS=False)), ("dense", {n: False for n in SWITCHES})):
            for n in SWITCHES:
                setattr(ops, n, on.get(n, saved[n] if n == "SKIP_ZERO_ROWS" else True))
            used[leg] = count = {}
            del passes[:]

            def counting(name, pred):
                fn = orig[name]

                def wrapped(*a, **kw):
                    if pred(a, kw):
                        count[name] = count.get(name, 0) + 1
                    return fn(*a, **kw)
                setattr(hip, name, wrapped)
            for name in ("ln_geglu_fwd", "ln_geglu_bwd", "layernorm_bwd"):
                counting(name, lambda a, kw: kw.get("ps") is not None)
            counting("resid_bwd", lambda a, kw: bool(kw.get("skip_zero_rows")))
            counting("live_mwindows_fwd", lambda a, kw: any(o is None for o in a[2]))     # an output that went without its fill
            counting("live_mwindows", lambda a, kw: len(a[2]) == 0)                      # a launch that only builds lists
            enc = one_peace_encoder_config(drop_path_rate=0.5, layer_scale_init_value=1e-1, checkpoint_activations=False, **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(BF).train()
            fl = FlatParameters(m)
            opt = FusedAdamW(fl, lr=5e-4, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05)
            poison_allocator(seg_rows + (sum(seg_rows),), H, F)
            opt.zero_grad()
            loss, _, _ = TriModalContrastiveCriterion(None, 0.0, lock_step=lock_step)(m, {"net_input": inp, "nsentences": B})
            loss.backward()
            torch.cuda.synchronize()
            grads = fl.grads.detach().clone()
            opt.step(grad_scale=1.0, clip_norm=3.0)
            torch.cuda.synchronize()
            res[leg] = (loss.detach().clone(), grads, fl.params.detach().clone())
            del m, fl, opt, loss
    finally:
        for n in SWITCHES:
            setattr(ops, n, saved[n])
        for n, fn in orig.items():
            setattr(hip, n, fn)
        TE.TransformerEncoder._draw_path_scales = orig_scales
        ops.set_recompute_cheap(old_cheap)
    print("launches that left rows out:", used)
    # the switch really changed the launches: layer 1's FFN forward (three segments; `cheap` re-creates LN_F(GeGLU) in backward), its
    # backward, the two LayerNorm backwards of the attention branch, four op_resid_bwd (attention + three FFN segments), the FFN
    # forward's fill without h0 | h1 and the attention backward's launch that only builds its list
    if lock_step:
        want = dict(ln_geglu_fwd=6 if cheap else 3, ln_geglu_bwd=3, layernorm_bwd=2, resid_bwd=4, live_mwindows_fwd=1, live_mwindows=1)
    else:  # three passes of one segment each: all three LayerNorm backwards skip, and both backward list launches fill nothing
        want = dict(ln_geglu_fwd=3, ln_geglu_bwd=3, layernorm_bwd=9, resid_bwd=6, live_mwindows_fwd=3, live_mwindows=6)
    assert used["rows"] == want, used["rows"]
    assert used["no_rows"] == {} and used["dense"] == {}, (used["no_rows"], used["dense"])
    for leg in ("no_rows", "dense"):
        for got, want, name in zip(res["rows"], res[leg], ("loss", "gradients", "updated parameters")):
            assert torch.equal(got, want), "%s differ between SKIP_ZERO_ROWS and the %s leg" % (name, leg)
    for t in res["rows"]:
        assert bool(torch.isfinite(t.float()).all())
    assert float(res["rows"][1].float().abs().sum()) > 0 and not torch.equal(res["rows"][2], torch.zeros_like(res["rows"][2]))
