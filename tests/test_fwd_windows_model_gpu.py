"""A training step with the forward GEMMs over row windows (ops.SKIP_ZERO_FWD) is the step with the dense launches, bit for bit."""
from types import SimpleNamespace

import pytest
import torch

from oracle import synth
from tests.model_util import TinyDictionary, load_synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


@pytest.mark.parametrize("mode", ["recompute", "keep", "cheap"])
def test_training_step_is_bit_identical_with_and_without_the_forward_windows(mode):
    """The step of tests/test_dgrad_windows_model_gpu.py: lock-step tri-modal, 2 layers (drop-path 0.4, fixed masks with runs of dropped
    neighbours): text 64 rows (aligned tiles), image 257 rows (one window per kept sample + the strided last row), audio 25 rows
    (aligned tiles).  64 samples per modality instead of that test's 48: with 48 the image segment has 12 336 rows, no multiple of 64,
    so gamma's gradient cannot come from the weight gradient (ops.dgamma_from_wgrad_ok), the branch output y is wanted and the dense
    launches take over by design -- at 48 no forward launch is listed and there is nothing to compare.  ops.SKIP_ZERO_FWD on and off
    (what ONEPEACE_SKIP_ZERO_FWD=0 sets) under the same masks give the same loss and the same flat gradient buffer.  Layer 0 has no
    multipliers and stays dense; layer 1 builds one list per branch and runs four listed launches per forward pass: q|k|v, out-proj +
    residual, the grouped wi_0 | wi_1, the grouped down-projection + residual.
    mode: recompute -- checkpoint_activations (that test's configuration): the forward and its recomputation in backward both run
    listed, FFN branch first in backward; keep -- activations kept; cheap -- kept, with ops.set_recompute_cheap(True): backward
    re-creates the LayerNorm rows from what the listed forward kept."""
    cheap = mode == "cheap"
    from one_peace_amd import hip, ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    cfg = dict(embed_dim=256, ffn_embed_dim=512, layers=2, attention_heads=4, image_rel_bucket_size=16, text_bucket_size=256,
               audio_bucket_size=512)
    B = 64
    inp = synth.synth_inputs(B, text_len=63, image_res=256, audio_samples=8000, vocab=1000)
    inp = {k: (v.to(DEV).to(BF) if v.is_floating_point() else v.to(DEV)) for k, v in inp.items()}
    orig, orig_live, orig_gemm = ops.SKIP_ZERO_FWD, hip.live_mwindows_fwd, hip.gemm_nt_windows_fwd
    orig_scales = TE.TransformerEncoder._draw_path_scales
    mask = torch.bernoulli(torch.full((2, 3 * B), 0.6), generator=torch.Generator(device="cpu").manual_seed(3)).bool()
    mask[0, :12] = False                 # text samples 0 .. 11 = three aligned tiles, attention branch
    mask[0, B + 4:B + 9] = False         # image samples 4 .. 8
    mask[1, 2 * B:2 * B + 24] = False    # audio samples 0 .. 23 = 600 rows: two aligned tiles, FFN branch
    mask[1, B + 20:B + 23] = False

    def fixed_scales(self, nb, device):
        assert nb == 3 * B
        return [(None, None), ((mask[0].float() / 0.6).to(device), (mask[1].float() / 0.6).to(device))]
    res, calls, launched = {}, {}, {}
    old_cheap = ops.set_recompute_cheap(cheap)
    try:
        TE.TransformerEncoder._draw_path_scales = fixed_scales
        for on in (True, False):
            ops.SKIP_ZERO_FWD = on
            calls[on], launched[on] = [], []

            def counted(segs, lists, outs, srcs, _on=on):
                out = orig_live(segs, lists, outs, srcs)
                calls[_on].append((out, [q is not None for q in srcs]))
                return out
            hip.live_mwindows_fwd = counted

            def listed(*a, _on=on, **kw):
                launched[_on].append((orig_gemm(*a, **kw), kw.get("epilogue", hip.EPI_BIAS), len(a[0])))
                return launched[_on][-1][0]
            hip.gemm_nt_windows_fwd = listed
            enc = one_peace_encoder_config(drop_path_rate=0.4, layer_scale_init_value=1e-1, checkpoint_activations=mode == "recompute", **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(BF).train()
            fl = FlatParameters(m)
            loss, _, _ = TriModalContrastiveCriterion(None, 0.0, lock_step=True)(m, {"net_input": inp, "nsentences": B})
            fl.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
            res[on] = (loss.detach().clone(), fl.grads.detach().clone())
    finally:
        ops.SKIP_ZERO_FWD, hip.live_mwindows_fwd, hip.gemm_nt_windows_fwd = orig, orig_live, orig_gemm
        TE.TransformerEncoder._draw_path_scales = orig_scales
        ops.set_recompute_cheap(old_cheap)
    assert not calls[False] and not launched[False]
    # every listed launch really ran on its list (False = the shape did not qualify and the dense launch took over)
    attn, ffn = [(True, hip.EPI_BIAS, 1), (True, hip.EPI_RESID, 1)], [(True, hip.EPI_BIAS, 3), (True, hip.EPI_RESID, 3)]
    assert launched[True] == attn + ffn + (ffn + attn if mode == "recompute" else []), launched[True]
    # one list per branch and pass of layer 1; each fills a plain output with +0 and the branch output with the residual input
    assert [(len(out), srcs) for out, srcs in calls[True]] == [(1, [False, True])] * (len(launched[True]) // 2)
    for out, _ in calls[True]:
        (lst, cnt), = out
        assert 0 < int(cnt.item()) < lst.numel() // 2, (int(cnt.item()), lst.numel() // 2)  # some window really was left out
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    assert float(res[True][1].float().abs().sum()) > 0 and bool(torch.isfinite(res[True][1].float()).all())
