"""Retrieval on the torch path (CPU): the Recall mirror against the reference's own eval_log (tests/golden/recall.pt, made by
tests/golden/make_recall_golden.py from one_peace/metrics/recall.py), the order of exact ties, the audio key names, a world-2 gloo run
through gather_variable, and the static checks of csrc/retrieval.hip (argument validation, ScratchSize 0, MFMA hazards)."""
import os
import shutil
import sys
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "recall.pt")


def recall_golden_inputs(fx):
    return fx["text_ids"], fx["text_emb"], fx["image_ids"], fx["image_emb"]


def recall_fp64(image_ids, image_logits, text_ids, text_logits):
    """recall.py:31-88 restated in fp64 on CPU (full score matrix, stable sort for the top 10)."""
    s = image_logits.double() @ text_logits.double().t()
    rank_txt = torch.sort(s, dim=1, descending=True, stable=True)[1][:, :10]
    rank_img = torch.sort(s.t(), dim=1, descending=True, stable=True)[1][:, :10]
    pt, pi = text_ids[rank_txt], image_ids[rank_img]
    n_img, n_txt = len(image_ids), len(text_ids)
    i2t = [pt[:, :r].eq(image_ids[:, None]).any(1).sum().item() for r in (1, 5, 10)]
    t2i = [pi[:, :r].eq(text_ids[:, None]).any(1).sum().item() for r in (1, 5, 10)]
    tr = [100.0 * c / n_img for c in i2t]
    ir = [100.0 * c / n_txt for c in t2i]
    tm, im = sum(tr) / 3, sum(ir) / 3
    return {"txt_r1": tr[0], "txt_r5": tr[1], "txt_r10": tr[2], "txt_r_mean": tm, "img_count": n_img, "img_r1": ir[0], "img_r5": ir[1],
            "img_r10": ir[2], "img_r_mean": im, "r_mean": (tm + im) / 2, "txt_count": n_txt,
            "predict_txt": dict(zip(image_ids.tolist(), pt.tolist())), "predict_img": dict(zip(text_ids.tolist(), pi.tolist()))}


def _recall(fx, modality="image", chunks=(slice(0, 7), slice(7, None))):
    from one_peace_amd.metrics import Recall
    text_ids, text_emb, image_ids, image_emb = recall_golden_inputs(fx)
    r = Recall(modality)
    r.initialize(text_ids, text_emb)
    for c in chunks:
        r.compute(image_ids[c], image_emb[c])
    return r


def test_recall_torch_path_reproduces_the_reference_eval_log():
    fx = torch.load(GOLDEN)
    log = _recall(fx).merge_results(output_predict=True)
    assert log == fx["eval_log"]
    assert log["img_count"] == 16 and log["txt_count"] == 65 and 0 < log["txt_r1"] < 100 and 0 < log["img_r1"] < 100
    assert log == recall_fp64(fx["image_ids"], fx["image_emb"], fx["text_ids"], fx["text_emb"])
    plain = _recall(fx).merge_results()
    assert plain["predict_txt"] == {} and plain["predict_img"] == {}
    assert {k: v for k, v in plain.items() if not k.startswith("predict")} == \
        {k: v for k, v in fx["eval_log"].items() if not k.startswith("predict")}


def test_recall_audio_names_the_query_side_audio():
    fx = torch.load(GOLDEN)
    log = _recall(fx, modality="audio").merge_results(output_predict=True)
    want = dict(fx["eval_log"])
    for key in list(want):
        if key.startswith("img"):
            want[key.replace("img", "audio")] = want.pop(key)
    assert log == want
    assert "audio_r1" in log and "audio_count" in log and "img_r1" not in log and "predict_img" in log


def test_similarity_topk_torch_path_orders_exact_ties_by_index():
    from one_peace_amd import ops
    g = torch.randint(-5, 6, (7, 16), generator=torch.Generator().manual_seed(0)).float()  # integer scores: exact in any order
    g = torch.cat([g, g[[3, 1]], g[[3]], torch.zeros(2, 16)])  # 7 = 3, 8 = 1, 9 = 3; 10, 11 zero rows
    q = g[[3, 1]].clone()
    vals, idx = ops.similarity_topk(q, g, 5)
    assert idx.dtype == torch.int64 and vals.dtype == torch.float32
    assert idx[0, :3].tolist() == [3, 7, 9] and idx[1, :2].tolist() == [1, 8]
    assert torch.equal(vals[0, 0], vals[0, 2])
    neg = -q
    _, idx = ops.similarity_topk(neg, g, 12)
    z = [i for i in idx[0].tolist() if i >= 10]
    assert z == [10, 11]  # the zero rows (score +0 and -0 alike) tie in index order
    with pytest.raises(ValueError):
        ops.similarity_topk(q, g, 13)


def test_hub_retrieve_is_similarity_topk():
    from one_peace_amd import ops
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    gen = torch.Generator().manual_seed(1)
    q, g = torch.randn(4, 32, generator=gen), torch.randn(50, 32, generator=gen)
    hub = OnePeaceHubInterface.__new__(OnePeaceHubInterface)
    v, i = hub.retrieve(q, g, k=10)
    rv, ri = ops.similarity_topk(q, g, 10)
    assert torch.equal(v, rv) and torch.equal(i, ri)
    assert torch.equal(ri, torch.topk(q @ g.t(), 10, dim=1)[1])


def _worker(rank, world, initfile, outdir):
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        from one_peace_amd.metrics import Recall, gather_variable
        fx = torch.load(GOLDEN)
        text_ids, text_emb, image_ids, image_emb = recall_golden_inputs(fx)
        img = [slice(0, 3), slice(3, 8)][rank]      # ranks hold 3 and 5 images ...
        txt = [slice(0, 7), slice(7, 19)][rank]     # ... and text shards of 7 and 12 rows
        t_ids = gather_variable(text_ids[txt])
        t_emb = gather_variable(text_emb[txt])
        assert torch.equal(t_ids, text_ids[:19]) and torch.equal(t_emb, text_emb[:19])
        r = Recall()
        r.initialize(t_ids, t_emb)
        r.compute(image_ids[img][:2], image_emb[img][:2])
        r.compute(image_ids[img][2:], image_emb[img][2:])
        torch.save(r.merge_results(output_predict=True), os.path.join(outdir, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_recall_world2_gloo_equals_single_process():
    fx = torch.load(GOLDEN)
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), d), nprocs=2, join=True)
        logs = [torch.load(os.path.join(d, "r%d.pt" % r)) for r in range(2)]
    text_ids, text_emb, image_ids, image_emb = recall_golden_inputs(fx)
    single = _recall({"text_ids": text_ids[:19], "text_emb": text_emb[:19], "image_ids": image_ids[:8], "image_emb": image_emb[:8]},
                     chunks=(slice(0, 8),)).merge_results(output_predict=True)
    assert logs[0] == single and logs[1] == single
    assert single["img_count"] == 8 and single["txt_count"] == 19 and len(next(iter(single["predict_img"].values()))) == 8


def test_sim_topk_entry_point_rejects_bad_arguments():
    from one_peace_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        pytest.skip("library not built")
    L = hip.lib()
    fake = 1 << 20  # never dereferenced: validation comes first
    for M, N, D, k, ldq in ((4, 100, 64, 0, 64), (4, 100, 64, 65, 64), (4, 5, 64, 6, 64), (4, 100, 48, 4, 48), (4, 100, 64, 4, 60)):
        rc = L.op_sim_topk(fake, ldq, fake, 64, M, N, D, k, fake, fake, None, 0, 0, None)
        assert rc == -22, (M, N, D, k)
        assert L.op_last_error().startswith(b"op_sim_topk")
    rc = L.op_sim_topk(fake, 64, fake, 64, 300, 3000, 64, 10, fake, fake, None, 0, 4, None)  # 4 splits need a workspace
    assert rc == -22 and b"workspace" in L.op_last_error()
    assert L.op_sim_topk_workspace_bytes(300, 3000, 10, 4) == 300 * 4 * 10 * 8
    assert L.op_sim_topk_workspace_bytes(300, 3000, 10, 1) == 0
    assert L.op_sim_topk_splits(5, 100, 0) == 1 and L.op_sim_topk_splits(1, 10 ** 6, 0) == 489
    assert L.op_abi_version() == 10


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
def test_retrieval_kernels_compile_without_scratch_and_pass_the_hazard_checker(tmp_path):
    sys.path.insert(0, ROOT)
    from tools import check_mfma_hazards as C
    isa = C.compile_isa(str(tmp_path), "retrieval")
    kernels, problems = C.check(isa)
    assert kernels == 2 and problems == [], problems[:5]
    usage = C.resource_usage(isa)
    names = sorted(usage)
    assert any("sim_topk_kernel" in n for n in names) and any("sim_topk_merge_kernel" in n for n in names)
    assert all(u.get("ScratchSize", 1) == 0 for u in usage.values()), usage
    assert "v_mfma_f32_16x16x32_bf16" in open(isa).read()
