"""The video backbone on the CPU against tests/golden/video.pt (the unmodified reference, fp32): strict loading under the reference's
keys, output and gradients for num_tadapter 1 and 2, the image model's features per frame after init_weights(), the freezing rule,
load_pretrained's designed missing keys, the recognizer's shapes and view averaging."""
import os

import pytest
import torch

from tests import video_util as V

ADAPTERS = ("T_Adapter", "S_Adapter", "MLP_Adapter")


def test_fixture_stays_under_the_size_limit():
    assert os.path.getsize(V.GOLDEN) < (1 << 20)


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_mirror_matches_the_reference_in_fp32(name):
    fx = V.fixture()
    case = fx["cases"][name]
    m = V.build(fx, case)   # (load_state_dict(strict=True) inside)
    assert set(m.state_dict()) == set(V.state_dict(fx, case))
    out, grads = V.run(m, fx)
    assert tuple(out.shape) == (2, fx["args"]["embed_dim"], fx["args"]["num_frames"], 1, 1)
    assert V.rel_fro(out, case["output"]) <= 1e-5, V.rel_fro(out, case["output"])
    names = set(case["grads"])
    assert all(any(a + "." in n for n in names) for a in ADAPTERS) and "image_adapter.temporal_embedding" in names
    assert "encoder.image_layer_norm.weight" in names and (case["num_tadapter"] == 2) == any("T_Adapter_in" in n for n in names)
    for key, want in case["grads"].items():
        assert float(want.abs().max()) > 0, key   # every path carries values
        assert V.rel_fro(grads[key], want) <= 1e-5, (key, V.rel_fro(grads[key], want))


def test_state_dict_round_trip_and_names():
    fx = V.fixture()
    case = fx["cases"]["tadapter2"]
    m = V.build(fx, case)
    sd, want = m.state_dict(), V.state_dict(fx, case)
    for k in ("image_adapter.rel_pos_table.weight", "image_adapter.rp_bucket", "image_adapter.cls_embedding", "image_adapter.pos_embed",
              "image_adapter.temporal_embedding", "image_adapter.embed_images.0.weight", "encoder.layers.1.image_ffn.3.bias",
              "encoder.layers.0.T_Adapter_in.D_fc1.weight", "encoder.layers.1.MLP_Adapter.D_fc2.bias", "encoder.image_layer_norm.weight"):
        assert k in sd, k
    assert not [k for k in sd if "position_idx" in k or "version" in k or "rel_pos_table_list" in k]
    for k, v in sd.items():
        assert torch.equal(v.float(), want[k]), k
    assert {n for n, _ in m.named_parameters()} == {k for k in sd if k != "image_adapter.rp_bucket"}
    assert m.no_weight_decay() == {"image_adapter.pos_embed", "image_adapter.cls_embedding", "image_adapter.temporal_embedding"}
    assert m.get_num_layers() == fx["args"]["layers"]
    outer = torch.nn.ModuleDict({"net": m})   # nested: the hooks honour the prefix
    assert set(outer.state_dict()) == {"net." + k for k in sd}
    outer.load_state_dict(outer.state_dict(), strict=True)
    from one_peace_amd.one_peace_vision import OnePeaceVideoViT
    with pytest.raises(NotImplementedError):
        OnePeaceVideoViT(**dict(fx["args"], rp_bias=True))


def _image_twin(fx, video_model):
    """The project's image classifier without global pooling carrying the video model's shared weights."""
    from one_peace_amd.one_peace_vision import OnePeaceViT
    args = {k: v for k, v in fx["args"].items() if k != "num_frames"}
    img = OnePeaceViT(global_pool=False, num_classes=3, **args)
    sd = {k.replace("encoder.image_layer_norm.", "encoder.layer_norm."): v for k, v in video_model.state_dict().items()
          if "Adapter" not in k and "temporal_embedding" not in k}
    res = img.load_state_dict(sd, strict=False)
    assert set(res.missing_keys) <= {"head.weight", "head.bias"} and not res.unexpected_keys, res
    return img.eval()


def test_fresh_adapters_compute_the_image_model_per_frame():
    from one_peace_amd.one_peace_vision import OnePeaceVideoViT
    fx = V.fixture()
    torch.manual_seed(5)
    m = OnePeaceVideoViT(num_tadapter=2, **fx["args"])
    m.init_weights()
    with torch.no_grad():
        m.image_adapter.rel_pos_table_list[0].weight.normal_(std=0.02)
    m.eval()
    assert float(m.image_adapter.temporal_embedding.detach().abs().max()) == 0.0
    for n, p in m.named_parameters():
        if "Adapter" in n and "D_fc2" in n:
            assert float(p.detach().abs().max()) == 0.0, n
    img = _image_twin(fx, m)
    video = fx["video"].float()
    B, C, T, H, W = video.shape
    with torch.no_grad():
        feats = m.forward_features(video)                                    # [N, B * T, D]
        frames = video.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
        want = img.forward_features(frames)                                  # [N, B * T, D], the final norm applied
        out = m(video)
    assert feats.shape == want.shape
    # the temporal pass still runs (T_Adapter's D_fc1 and the attention are live): its zero D_fc2 is what makes the frames independent
    assert V.rel_fro(feats, want) <= 1e-5, V.rel_fro(feats, want)
    assert torch.equal(out[:, :, :, 0, 0], feats[0].view(B, T, -1).permute(0, 2, 1))


def test_freeze_for_adapters_leaves_the_reference_set_trainable():
    from one_peace_amd.one_peace_vision import VideoRecognizer, freeze_for_adapters
    fx = V.fixture()
    rec = VideoRecognizer(V.build(fx, fx["cases"]["tadapter2"]), num_classes=7)
    kept = set(freeze_for_adapters(rec))
    want = {n for n, _ in rec.named_parameters()
            if "temporal_embedding" in n or "image_layer_norm" in n or "cls_head" in n or "Adapter" in n}   # video/train.py:189
    assert kept == want == {n for n, p in rec.named_parameters() if p.requires_grad}
    assert "cls_head.weight" in kept and "backbone.image_adapter.temporal_embedding" in kept and "backbone.encoder.image_layer_norm.bias" in kept
    assert sum("T_Adapter_in" in n for n in kept) == 4 * fx["args"]["layers"]
    assert not [n for n in kept if "self_attn" in n or "image_ffn" in n or "gamma" in n or "pos_embed" in n or "rel_pos" in n]
    # a step: gradients exactly for the kept set
    out = rec(fx["video"].float())
    assert tuple(out.shape) == (2, 7)
    out.sum().backward()
    assert {n for n, p in rec.named_parameters() if p.grad is not None} == kept


def test_load_pretrained_reports_the_designed_missing_keys():
    from one_peace_amd.one_peace_vision import OnePeaceVideoViT, load_pretrained_video
    fx = V.fixture()
    src = V.build(fx, fx["cases"]["tadapter1"])
    # what convert_to_vision hands over: the adapter and the layers, the table under the pretraining model's name, no final norm
    ckpt = {k.replace("rel_pos_table.weight", "rel_pos_table_list.0.weight"): v.clone() for k, v in src.state_dict().items()
            if "Adapter" not in k and "temporal_embedding" not in k and "image_layer_norm" not in k}
    assert "image_adapter.rel_pos_table_list.0.weight" in ckpt
    before = {k: v.clone() for k, v in ckpt.items()}
    torch.manual_seed(9)
    m = OnePeaceVideoViT(num_tadapter=2, **fx["args"])
    m.init_weights()
    missing, unexpected = load_pretrained_video(m, ckpt)
    designed = {n for n, _ in m.named_parameters() if "Adapter" in n} | {"image_adapter.temporal_embedding", "encoder.image_layer_norm.weight",
                                                                           "encoder.image_layer_norm.bias"}
    assert set(missing) == designed and len(missing) == len(designed) and not unexpected
    assert set(ckpt) == set(before) and all(torch.equal(ckpt[k], before[k]) for k in before)   # the argument is left as it is
    got = m.state_dict()
    for k, v in src.state_dict().items():
        if k not in designed:
            assert torch.equal(got[k], v), k
    # either spelling of the table, and a nested {'state_dict': ...}
    ckpt2 = {"state_dict": {k.replace("rel_pos_table_list.0.weight", "rel_pos_table.weight"): v for k, v in ckpt.items()}}
    m2 = OnePeaceVideoViT(num_tadapter=2, **fx["args"])
    missing2, unexpected2 = load_pretrained_video(m2, ckpt2)
    assert set(missing2) == designed and not unexpected2
    assert torch.equal(m2.state_dict()["image_adapter.rel_pos_table.weight"], src.state_dict()["image_adapter.rel_pos_table.weight"])


def test_video_recognizer_shapes_and_view_averaging():
    from one_peace_amd.one_peace_vision import VideoRecognizer
    fx = V.fixture()
    rec = VideoRecognizer(V.build(fx, fx["cases"]["tadapter1"]), num_classes=5, dropout_ratio=0.5).eval()
    with torch.no_grad():
        torch.nn.init.normal_(rec.cls_head.weight, std=0.1)   # moderate scores: the two averages differ
        video = fx["video"].float()
        views = torch.stack([video, video.flip(-1), video.roll(1, 2)], dim=1)          # [B, 3 views, C, T, H, W]
        scores = torch.stack([rec(views[:, i]) for i in range(3)], dim=1)              # [B, 3, classes]
        got = rec.forward_test(views)
        feat = rec.backbone(video)
    assert tuple(got.shape) == (2, 5) and torch.allclose(got.sum(-1), torch.ones(2), atol=1e-6)
    want = torch.softmax(scores, dim=-1).mean(dim=1)   # average_clips='prob': probabilities, not scores
    assert torch.allclose(got, want, atol=1e-6) and not torch.allclose(got, torch.softmax(scores.mean(dim=1), dim=-1), atol=1e-5)
    assert torch.allclose(scores[:, 0], rec.cls_head(feat[:, :, :, 0, 0].mean(dim=2)), atol=1e-6)   # eval: dropout is the identity


def test_training_mode_takes_three_draws_per_layer_and_checkpoint_recomputes():
    from one_peace_amd.one_peace_vision import video_vit
    fx = V.fixture()
    m = V.build(fx, fx["cases"]["tadapter1"], drop_path_rate=0.5, use_checkpoint=True).train()
    rates = [layer.drop_path_prob for layer in m.encoder.layers]
    assert rates[0] == 0.0 and abs(rates[-1] - 0.5) < 1e-6
    calls, real = [], video_vit._drop_path_rows
    video_vit._drop_path_rows = lambda x, p, training: calls.append((tuple(x.shape), p)) or real(x, p, training)
    try:
        with torch.no_grad():
            m(fx["video"].float())
    finally:
        video_vit._drop_path_rows = real
    assert len(calls) == 3 * len(rates) and all(shape[0] == 2 * fx["args"]["num_frames"] for shape, _ in calls)   # rows = frames
    torch.manual_seed(0)
    x = torch.ones(64, 3, 8)
    y = real(x, 0.25, True)
    per_frame = y[:, 0, 0]
    assert torch.equal(y, per_frame.view(-1, 1, 1).expand_as(y)) and all(v == 0.0 or abs(v - 1.0 / 0.75) < 1e-6 for v in per_frame.tolist())
    assert 0 < int((per_frame == 0).sum()) < 64
    out = m(fx["video"].float())   # through torch.utils.checkpoint
    out.sum().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
