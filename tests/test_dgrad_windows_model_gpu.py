"""A training step with the input gradients over row windows (ops.SKIP_ZERO_DGRAD) is the step with the dense launches, bit for bit."""
from types import SimpleNamespace

import pytest
import torch

from oracle import synth
from tests.model_util import TinyDictionary, load_synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def test_training_step_is_bit_identical_with_and_without_the_windows():
    """One lock-step tri-modal training step of a 2-layer model (drop-path 0.4, fixed seed), 48 samples per modality: text 64 rows
    (aligned tiles), image 257 rows (256 x 256 pixels: one window per kept sample + the strided last row), audio 25 rows (aligned
    tiles).  Every segment has more than 1024 rows, so that the dense launches sum K in one piece and the lists apply.
    ops.SKIP_ZERO_DGRAD on and off (what ONEPEACE_SKIP_ZERO_DGRAD=0 sets) under the same masks give the same loss and the same flat
    gradient buffer.  The masks are Bernoulli(0.6) draws plus runs of dropped neighbours, so that whole windows and whole aligned tiles
    are certain to be left out."""
    from one_peace_amd import hip, ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    cfg = dict(embed_dim=256, ffn_embed_dim=512, layers=2, attention_heads=4, image_rel_bucket_size=16, text_bucket_size=256,
               audio_bucket_size=512)
    B = 48
    inp = synth.synth_inputs(B, text_len=63, image_res=256, audio_samples=8000, vocab=1000)
    inp = {k: (v.to(DEV).to(BF) if v.is_floating_point() else v.to(DEV)) for k, v in inp.items()}
    orig, orig_live, orig_scales = ops.SKIP_ZERO_DGRAD, hip.live_mwindows, TE.TransformerEncoder._draw_path_scales
    orig_gemm = hip.gemm_nt_windows
    mask = torch.bernoulli(torch.full((2, 3 * B), 0.6), generator=torch.Generator(device="cpu").manual_seed(3)).bool()
    mask[0, :12] = False                 # text samples 0 .. 11 = three aligned tiles, attention branch
    mask[0, B + 4:B + 9] = False         # image samples 4 .. 8
    mask[1, 2 * B:2 * B + 24] = False    # audio samples 0 .. 23 = 600 rows: two aligned tiles, FFN branch
    mask[1, B + 20:B + 23] = False

    def fixed_scales(self, nb, device):
        assert nb == 3 * B
        return [(None, None), ((mask[0].float() / 0.6).to(device), (mask[1].float() / 0.6).to(device))]
    res, calls, launched = {}, {}, {}
    try:
        TE.TransformerEncoder._draw_path_scales = fixed_scales
        for on in (True, False):
            ops.SKIP_ZERO_DGRAD = on
            calls[on] = []

            def counted(segs, lists, outs, _on=on):
                out = orig_live(segs, lists, outs)
                calls[_on].append(out)
                return out
            hip.live_mwindows = counted
            launched[on] = []

            def listed(*a, _on=on, **kw):
                launched[_on].append(orig_gemm(*a, **kw))
                return launched[_on][-1]
            hip.gemm_nt_windows = listed
            enc = one_peace_encoder_config(drop_path_rate=0.4, layer_scale_init_value=1e-1, **cfg)
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
        ops.SKIP_ZERO_DGRAD, hip.live_mwindows, TE.TransformerEncoder._draw_path_scales = orig, orig_live, orig_scales
        hip.gemm_nt_windows = orig_gemm
    assert not calls[False] and not launched[False]
    # every listed GEMM really ran on its list (False = the shape did not qualify and the dense launch took over): out-proj and q|k|v,
    # the three down-projections, the grouped wi_0 | wi_1 launch
    assert launched[True] == [True] * 6, launched[True]
    # layer 0 has drop-path 0 (linspace), layer 1 has 0.4: one launch for its attention branch (one list), one for its FFN branch
    # (a list per segment and the grouped one)
    assert sorted(len(out) for out in calls[True]) == [1, 4], [len(out) for out in calls[True]]
    for out in calls[True]:
        counts = [(int(cnt.item()), lst.numel() // 2) for lst, cnt in out]
        assert all(0 < c <= n for c, n in counts) and any(c < n for c, n in counts), counts  # some window really was left out
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    assert float(res[True][1].float().abs().sum()) > 0
