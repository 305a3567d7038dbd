"""The vision-branch classifier on the CPU against tests/golden/vision.pt (the unmodified reference, fp32): strict loading under the
reference's keys, logits and gradients, checkpoint conversion and loading, the layer-decay groups; token_mean_norm_torch against the
three reference lines; the fp64 restatement of tests/tokenpool_ref.py against torch.autograd."""
import os
from types import SimpleNamespace

import pytest
import torch

from tests import tokenpool_ref as T
from tests import vision_util as V


def test_fixture_stays_under_the_size_limit():
    assert os.path.getsize(V.GOLDEN) < (1 << 20)


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_mirror_matches_the_reference_in_fp32(name):
    fx = V.fixture()
    case = fx["cases"][name]
    m = V.build(fx, case)   # (load_state_dict(strict=True) inside)
    assert set(m.state_dict()) == set(case["state_dict"])
    logits, grads = V.run(m, fx)
    assert V.rel_fro(logits, case["logits"]) <= 1e-5, V.rel_fro(logits, case["logits"])
    assert len(case["grads"]) == (4 if case["global_pool"] else 3)
    for key, want in case["grads"].items():
        assert V.rel_fro(grads[key], want) <= 1e-5, (key, V.rel_fro(grads[key], want))


def test_state_dict_round_trip_and_names():
    fx = V.fixture()
    case = fx["cases"]["global_pool"]
    m = V.build(fx, case)
    sd = m.state_dict()
    for k in ("image_adapter.rel_pos_table.weight", "image_adapter.rp_bucket", "image_adapter.cls_embedding", "image_adapter.pos_embed",
              "image_adapter.embed_images.0.weight", "encoder.layers.1.image_ffn.3.bias", "fc_norm.weight", "head.bias"):
        assert k in sd, k
    assert not [k for k in sd if "position_idx" in k or "version" in k or "rel_pos_table_list" in k or "image_layer_norm" in k]
    for k, v in sd.items():
        assert torch.equal(v.float(), case["state_dict"][k].float()), k
    assert {n for n, _ in m.named_parameters()} == {k for k in sd if k != "image_adapter.rp_bucket"}
    assert m.no_weight_decay() == {"image_adapter.pos_embed", "image_adapter.cls_embedding"}
    cls = V.build(fx, fx["cases"]["cls_token"])
    assert "encoder.layer_norm.weight" in cls.state_dict() and "fc_norm.weight" not in cls.state_dict()
    # nested: the hooks honour the prefix
    outer = torch.nn.ModuleDict({"net": m})
    assert set(outer.state_dict()) == {"net." + k for k in sd}
    outer.load_state_dict(outer.state_dict(), strict=True)


def test_head_initialisation_and_unsupported_arguments():
    from one_peace_amd.one_peace_vision import OnePeaceViT
    fx = V.fixture()
    torch.manual_seed(3)
    m = OnePeaceViT(**dict(fx["args"], init_scale=0.5))
    assert float(m.head.weight.abs().max()) <= 0.5 * 2.0 and 0.005 < float(m.head.weight.std()) < 0.015   # trunc_normal_(std=.02) * 0.5
    assert float(m.head.bias.abs().max()) == 0.0
    with pytest.raises(NotImplementedError):
        OnePeaceViT(**dict(fx["args"], rp_bias=True))
    ck = OnePeaceViT(**dict(fx["args"], use_checkpoint=True))
    assert ck.cfg.checkpoint_activations is True


def _tiny_pretrain(args):
    from one_peace_amd.one_peace.one_peace_pretrain import OnePeacePretrainModel
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from tests.model_util import TinyDictionary
    kw = dict(embed_dim=args["embed_dim"], ffn_embed_dim=args["ffn_embed_dim"], attention_heads=args["attention_heads"],
              image_bucket_size=args["bucket_size"], image_rel_bucket_size=args["bucket_size"], use_audio_moe=False, drop_path_rate=0.0,
              checkpoint_activations=False)
    cfg = SimpleNamespace(encoder=one_peace_encoder_config(layers=args["layers"], **kw), decoder=one_peace_encoder_config(layers=1, **kw),
                          logit_scale_init=1 / 0.07, reset_logit_scale=False, stage2_pretrain=False, copy_rel_pos_table=False)
    torch.manual_seed(1)
    return OnePeacePretrainModel(cfg, TinyDictionary(100))


def test_convert_to_vision_and_load_pretrained():
    from one_peace_amd.one_peace_vision import OnePeaceViT, convert_to_vision, load_pretrained
    fx = V.fixture()
    pre = _tiny_pretrain(fx["args"])
    full = pre.state_dict()
    assert any("text" in k for k in full) and any("decoder" in k for k in full) and "image_proj.weight" in full
    before = dict(full)
    vis = convert_to_vision(full)
    assert dict(full) == before and all(torch.equal(full[k], before[k]) for k in full)   # the argument is left alone
    assert "image_adapter.rel_pos_table_list.0.weight" in vis and "encoder.layers.0.self_attn.q_proj.weight" in vis
    assert not [k for k in vis if any(t in k for t in ("text", "audio", "decoder", "mask", "logit_scale", "version", "image_proj"))]
    assert not [k for k in vis if "fusion_model" in k or "encoder_wrapper" in k or "image_layer_norm" in k]
    torch.manual_seed(2)
    m = OnePeaceViT(global_pool=True, **fx["args"])
    missing, unexpected = load_pretrained(m, vis)
    assert unexpected == [], unexpected
    assert sorted(missing) == ["fc_norm.bias", "fc_norm.weight", "head.bias", "head.weight"], missing
    sd = m.state_dict()
    # exactly the keys the model consumes: everything but its own rp_bucket, fc_norm and head came from the checkpoint
    consumed = {("image_adapter.rel_pos_table.weight" if k == "image_adapter.rel_pos_table_list.0.weight" else k) for k in vis}
    consumed.discard("image_adapter.rp_bucket")
    consumed.discard("image_adapter.position_idx")
    assert consumed == {k for k in sd if k.split(".")[0] not in ("fc_norm", "head") and k != "image_adapter.rp_bucket"}, consumed ^ set(sd)
    assert torch.equal(sd["encoder.layers.1.image_ffn.3.weight"], full["encoder_wrapper.fusion_model.layers.1.image_ffn.3.weight"])
    assert torch.equal(sd["image_adapter.rel_pos_table.weight"], full["encoder_wrapper.image_adapter.rel_pos_table_list.0.weight"])
    assert torch.equal(sd["image_adapter.pos_embed"], full["encoder_wrapper.image_adapter.pos_embed"])
    # the other spelling of the table, as a checkpoint saved by the reference's own model has it
    renamed = {("image_adapter.rel_pos_table.weight" if k == "image_adapter.rel_pos_table_list.0.weight" else k): v for k, v in vis.items()}
    m2 = OnePeaceViT(global_pool=True, **fx["args"])
    missing2, unexpected2 = load_pretrained(m2, renamed)
    assert unexpected2 == [] and sorted(missing2) == sorted(missing)
    assert torch.equal(m2.state_dict()["image_adapter.rel_pos_table.weight"], sd["image_adapter.rel_pos_table.weight"])
    out = m2.eval()(fx["images"].float())
    assert tuple(out.shape) == (2, fx["args"]["num_classes"]) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_param_groups_lrd_reproduces_the_recorded_groups(name):
    from one_peace_amd.one_peace_vision import get_layer_id_for_vit, param_groups_lrd, vision_param_groups
    fx = V.fixture()
    case = fx["cases"][name]
    m = V.build(fx, case)
    names = {id(p): n for n, p in m.named_parameters()}
    groups = param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
    got = [{"lr_scale": g["lr_scale"], "weight_decay": g["weight_decay"], "params": [names[id(p)] for p in g["params"]]} for g in groups]
    assert len(got) == len(case["groups"])
    for mine, want in zip(got, case["groups"]):
        assert mine["params"] == want["params"]
        assert mine["lr_scale"] == pytest.approx(want["lr_scale"], rel=1e-12) and mine["weight_decay"] == want["weight_decay"]
    L = len(m.encoder.layers) + 1
    assert get_layer_id_for_vit("image_adapter.pos_embed", L) == 0 and get_layer_id_for_vit("encoder.layers.1.gamma_1", L) == 2
    assert get_layer_id_for_vit("head.weight", L) == L and get_layer_id_for_vit("encoder.layer_norm.weight", L) == L
    # the callables for FlatParameters / FusedAdamW say the same, also for the composed modules' own names
    no_decay, lr_scale = vision_param_groups(m, layer_decay=0.75)
    for g in case["groups"]:
        for n in g["params"]:
            p = dict(m.named_parameters())[n]
            assert lr_scale(n, p) == pytest.approx(g["lr_scale"], rel=1e-12) and no_decay(n, p) == (g["weight_decay"] == 0.0), n
    assert lr_scale("image_adapter.rel_pos_table_list.0.weight", None) == pytest.approx(0.75 ** L)


def test_token_mean_norm_torch_is_the_three_reference_lines():
    from one_peace_amd import ops
    torch.manual_seed(0)
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(3, 17, 72).to(dtype)
        norm = torch.nn.LayerNorm(72).to(dtype)
        with torch.no_grad():
            norm.weight.normal_()
            norm.bias.normal_()
        want = norm(x[:, 1:, :].mean(dim=1))       # models_vit.py:432-433
        got = ops.token_mean_norm_torch(x, norm.weight, norm.bias, norm.eps)
        assert got.dtype == dtype and torch.equal(got, want)
        assert torch.equal(ops.token_mean_norm(x, norm.weight, norm.bias, norm.eps), want)   # the CPU takes the torch route
    with pytest.raises(ValueError):
        ops.token_mean_norm(torch.zeros(2, 1, 8), None, None)


@pytest.mark.parametrize("shape", [(1, 2, 8), (3, 17, 72), (5, 130, 264)])
def test_fp64_restatement_agrees_with_autograd(shape):
    from one_peace_amd import ops
    B, S, H = shape
    x, dy, w, b = T.make_inputs(B, S, H)
    fwd = T.forward_ref(x, w, b, 1e-5)
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, b))
    y = ops.token_mean_norm_torch(xg, wg, bg, 1e-5)
    y.backward(dy)
    assert float((fwd["y"][0] - y.detach()).abs().max()) <= 1e-12
    bwd = T.backward_ref(dy, fwd["pooled"][0], w, fwd["mean"][0], fwd["rstd"][0], S)
    assert float((bwd["dx"][0] - xg.grad).abs().max()) <= 1e-12
    assert bool((bwd["dx"][0][:, 0] == 0).all())
    assert float((bwd["dw_part"][0] - wg.grad).abs().max()) <= 1e-11 and float((bwd["db_part"][0] - bg.grad).abs().max()) <= 1e-11
    for out in list(fwd.values()) + list(bwd.values()):   # budgets: finite, non-negative, zero only where nothing is computed
        assert bool(torch.isfinite(out[1]).all()) and bool(torch.isfinite(out[2]).all()) and bool((out[1] >= 0).all()) and bool((out[2] >= 0).all())
    assert T.splits(2) == (64, 1) and T.splits(257) == (64, 4) and T.splits(1025) == (64, 16) and T.splits(130) == (64, 3)
    assert T.splits(65536) == (4096, 16)
