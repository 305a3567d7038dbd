"""op_sim_topk (csrc/retrieval.hip) and the Recall mirror on the device: top-k against torch fp64 scores, the total order (exact ties,
NaN / inf), bit-identity across split counts and runs, no materialised score matrix, and Recall against the reference's eval_log."""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.test_retrieval_cpu import recall_fp64, recall_golden_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda"


def hipmod():
    from one_peace_amd import hip
    return hip


def unit_bf16(rows, D, seed):
    x = torch.randn(rows, D, generator=torch.Generator().manual_seed(seed))
    return F.normalize(x, dim=1).to(torch.bfloat16).to(DEV)


def check_topk(q, g, k, vals, idx):
    """vals within 2e-6 sqrt(D) of the fp64 top-k; indices equal wherever the fp64 gap to the neighbouring ranks exceeds 1e-4, and
    elsewhere every returned index scores (fp64) at least the k-th fp64 score minus the tolerance."""
    D = q.shape[1]
    tol = 2e-6 * D ** 0.5
    ref = q.double() @ g.double().t()
    kk = min(k + 1, g.shape[0])
    rv, ri = torch.topk(ref, kk, dim=1)
    assert vals.shape == (q.shape[0], k) and idx.shape == (q.shape[0], k) and idx.dtype == torch.int64
    assert (vals.double() - rv[:, :k]).abs().max().item() <= tol
    assert bool((vals[:, :-1] >= vals[:, 1:]).all())
    got = ref.gather(1, idx)
    assert (vals.double() - got).abs().max().item() <= tol
    gap = torch.full_like(rv[:, :k], float("inf"))
    gap[:, 1:] = rv[:, :k - 1] - rv[:, 1:k]
    if kk > k:
        gap = torch.minimum(gap, rv[:, :k] - rv[:, 1:k + 1])
    else:
        gap[:, :-1] = torch.minimum(gap[:, :-1], rv[:, :k - 1] - rv[:, 1:k])
    sure = gap > 1e-4
    assert torch.equal(idx[sure], ri[:, :k][sure])
    assert bool((got >= rv[:, k - 1:k] - tol).all())
    assert len(set(idx[0].tolist())) == k


@pytest.mark.parametrize("M,N,D,k", [(1, 50, 64, 1), (37, 1000, 256, 10), (5000, 25010, 1536, 10), (25010, 5000, 1536, 10),
                                     (3, 300000, 1536, 16), (130, 389, 96, 7), (5, 300, 40, 3), (200, 64, 32, 64)])
def test_sim_topk_against_fp64(M, N, D, k):
    hip = hipmod()
    q, g = unit_bf16(M, D, 1), unit_bf16(N, D, 2)
    vals, idx = hip.sim_topk(q, g, k)
    torch.cuda.synchronize()
    check_topk(q, g, k, vals, idx)


def test_sim_topk_ties_splits_and_runs_are_bit_identical():
    """Duplicated gallery rows give exactly equal scores: they come back in ascending index order.  Two split counts and two runs of
    the same call give the same bits."""
    hip = hipmod()
    base, M, k = 1000, 300, 16
    q = unit_bf16(M, 256, 3)
    g = unit_bf16(base, 256, 4).repeat(3, 1).contiguous()  # rows i, i + 1000, i + 2000 identical
    L = hip.lib()
    s_auto = L.op_sim_topk_splits(M, g.shape[0], 0)
    assert L.op_sim_topk_splits(M, g.shape[0], 1) == 1 and L.op_sim_topk_splits(M, g.shape[0], 13) == 12 and s_auto > 1
    v1, i1 = hip.sim_topk(q, g, k, splits=1)
    v2, i2 = hip.sim_topk(q, g, k, splits=13)
    v3, i3 = hip.sim_topk(q, g, k, splits=13)
    v4, i4 = hip.sim_topk(q, g, k)
    torch.cuda.synchronize()
    for v, i in ((v2, i2), (v3, i3), (v4, i4)):
        assert torch.equal(v1.view(torch.int32), v.view(torch.int32)) and torch.equal(i1, i)
    # every triple is complete and ordered: positions 3j, 3j+1, 3j+2 hold i, i + 1000, i + 2000 with the same score
    for j in range(0, 15, 3):
        assert torch.equal(v1[:, j], v1[:, j + 1]) and torch.equal(v1[:, j], v1[:, j + 2])
        assert torch.equal(i1[:, j + 1], i1[:, j] + base) and torch.equal(i1[:, j + 2], i1[:, j] + 2 * base)
    assert bool((i1[:, ::3][:, :5] < base).all())
    check_topk(q, g, k, v1, i1)


def test_sim_topk_nan_and_inf_rows():
    from one_peace_amd import ops
    hip = hipmod()
    gen = torch.Generator().manual_seed(5)
    q = (torch.rand(4, 64, generator=gen) + 0.1).to(torch.bfloat16)
    g = (torch.rand(40, 64, generator=gen) + 0.1)
    g[5], g[33], g[17], g[30] = float("nan"), float("nan"), float("inf"), float("-inf")
    g = g.to(torch.bfloat16)
    for splits in (1, 0):
        vals, idx = hip.sim_topk(q.to(DEV), g.to(DEV), 40, splits=splits)
        vals, idx = vals.cpu(), idx.cpu()
        assert (idx[:, :3] == torch.tensor([5, 33, 17])).all() and (idx[:, -1] == 30).all()
        assert torch.isnan(vals[:, :2]).all() and (vals[:, 2] == float("inf")).all() and (vals[:, -1] == float("-inf")).all()
        assert torch.isfinite(vals[:, 3:-1]).all()
        cv, ci = ops.similarity_topk(q.float(), g.float(), 40)
        assert torch.equal(ci, idx)  # the torch path: the same order


def test_sim_topk_never_materialises_the_scores():
    hip = hipmod()
    M, N, D = 4096, 300000, 1536
    q, g = unit_bf16(M, D, 6), unit_bf16(N, D, 7)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    vals, idx = hip.sim_topk(q, g, 10)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    assert grown < M * N * 4 // 8, grown
    assert vals.shape == (M, 10)


def test_sim_topk_rejects_what_it_does_not_take():
    hip = hipmod()
    q, g = unit_bf16(4, 64, 8), unit_bf16(70, 64, 9)
    with pytest.raises(ValueError):
        hip.sim_topk(q, g, 65)
    with pytest.raises(ValueError):
        hip.sim_topk(q, g[:5], 6)


def test_recall_on_device_matches_the_reference_eval_log(golden_dir):
    from one_peace_amd.metrics import Recall
    fx = torch.load(os.path.join(golden_dir, "recall.pt"))
    text_ids, text_emb, image_ids, image_emb = recall_golden_inputs(fx)
    r = Recall()
    r.initialize(text_ids.to(DEV), text_emb.to(torch.bfloat16).to(DEV))
    for part in (slice(0, 7), slice(7, None)):
        r.compute(image_ids[part].to(DEV), image_emb[part].to(torch.bfloat16).to(DEV))
    log = r.merge_results(output_predict=True)
    assert log == fx["eval_log"]


def test_recall_end_to_end_from_a_micro_pretrain_model():
    """Texts and images encoded by a micro OnePeacePretrainModel on the HIP path; Recall equals a CPU fp64 restatement of recall.py
    on the same embeddings."""
    from types import SimpleNamespace
    from one_peace_amd.metrics import Recall
    from one_peace_amd.one_peace.one_peace_pretrain import OnePeacePretrainModel
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from oracle import synth
    from tests.model_util import TinyDictionary, load_synth
    enc = one_peace_encoder_config(embed_dim=128, ffn_embed_dim=256, layers=2, attention_heads=2, drop_path_rate=0.0,
                                   image_rel_bucket_size=4, use_audio_moe=False)
    dec = one_peace_encoder_config(embed_dim=64, ffn_embed_dim=128, layers=1, attention_heads=1, drop_path_rate=0.0,
                                   use_audio_moe=False)
    dec.text_adapter.use_attn_bias = dec.image_adapter.use_attn_bias = False
    dec.image_adapter.vision_encoder_type = "none"
    cfg = SimpleNamespace(encoder=enc, decoder=dec, reset_logit_scale=False, logit_scale_init=1 / 0.07, stage2_pretrain=False)
    torch.manual_seed(0)
    model = load_synth(OnePeacePretrainModel(cfg, TinyDictionary(1000))).to(DEV).to(torch.bfloat16).eval()
    n_img, per = 12, 3
    inp = synth.synth_inputs(n_img * per, text_len=15, image_res=64, audio_samples=8000, vocab=1000)
    with torch.no_grad():
        text_logits, _ = model(src_tokens=inp["src_tokens"].to(DEV), encoder_type="text")
        image_logits, _ = model(src_images=inp["src_images"][:n_img].to(DEV).to(torch.bfloat16), encoder_type="image")
    assert text_logits.dtype == torch.bfloat16 and image_logits.is_cuda
    text_ids = torch.arange(n_img).repeat_interleave(per).to(DEV)
    image_ids = torch.arange(n_img).to(DEV)
    r = Recall()
    r.initialize(text_ids, text_logits)
    r.compute(image_ids, image_logits)
    log = r.merge_results(output_predict=True)
    ref = recall_fp64(image_ids.cpu(), image_logits.cpu(), text_ids.cpu(), text_logits.cpu())
    assert log == ref
