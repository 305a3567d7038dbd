"""OnePeaceDetViT without a GPU: the fixture of the unmodified reference (tests/golden/det.pt) reproduced in fp32 -- output and every
recorded gradient within 1e-5 relative Frobenius, the video test's gate --, the reference's state-dict keys and a strict load, the
checkpoint loading of load_pretrained_det from a 16-bucket state dict with the pretraining name of the table, get_onepeace_lr_decay_rate
on the names the reference's docstring covers, and rp_bias=True refused."""
import pytest
import torch

from tests import det_util as D

TOL = 1e-5


def test_fixture_is_reproduced_in_fp32():
    fx = D.fixture()
    m = D.build(fx)
    out, grads = D.run(m, fx)
    assert tuple(out.shape) == tuple(fx["output"].shape) == (1, fx["args"]["embed_dim"], 32, 32)
    errs = {"output": D.rel_fro(out, fx["output"])}
    need = ("rel_pos_h", "rel_pos_w", "rel_pos_table.weight", "pos_embed", "q_proj.bias", "v_proj.bias", "gamma_1", "k_proj.weight")
    assert all(any(n.endswith(s) for n in fx["grad_names"]) for s in need)
    assert sum("rel_pos_h" in n or "rel_pos_w" in n for n in fx["grad_names"]) == 4          # both tables of both layers
    for n in fx["grad_names"]:
        errs[n] = D.rel_fro(grads[n], fx["grads"][n])
    assert all(e <= TOL for e in errs.values()), errs


def test_state_dict_keys_are_the_references_and_load_strictly():
    from one_peace_amd.one_peace_vision import OnePeaceDetViT
    fx = D.fixture()
    m = OnePeaceDetViT(**fx["args"])
    assert list(m.state_dict().keys()) == fx["state_dict_keys"]
    assert sorted(n for n, _ in m.named_parameters()) == sorted(k for k in fx["state_dict_keys"] if k not in D.BUCKETS)
    for k in D.BUCKETS:   # the index arithmetic of the two buffers the fixture cannot hold in full
        own = m.state_dict()[k]
        assert all(torch.equal(own[i], row.long()) for i, row in fx["bucket_rows"][k].items()) and int(own.sum()) == fx["bucket_sums"][k]
    sd = D.state_dict(fx, m)
    assert set(sd) == set(fx["state_dict_keys"])
    m.load_state_dict(sd, strict=True)
    layer0, layer1 = m.encoder.layers
    assert layer0.window_size == 16 and layer1.window_size == 0
    assert tuple(layer0.self_attn.rel_pos_h.shape) == (31, 64) and tuple(layer1.self_attn.rel_pos_w.shape) == (63, 64)


def test_load_pretrained_from_a_16_bucket_checkpoint():
    from one_peace_amd.one_peace_vision import OnePeaceDetViT, load_pretrained_det
    fx = D.fixture()
    torch.manual_seed(1)
    m = OnePeaceDetViT(**fx["args"])
    dim = fx["args"]["embed_dim"]
    ck = {k: v.float().clone() for k, v in fx["state_dict"].items() if "rel_pos" not in k}
    ck["image_adapter.pos_embed"] = torch.randn(16 * 16 + 1, dim)
    ck["image_adapter.rel_pos_table_list.0.weight"] = torch.randn(31 * 31 + 3, fx["args"]["attention_heads"])
    ck["image_adapter.rp_bucket"] = torch.zeros(257, 257, dtype=torch.long)
    before = {k: v.clone() for k, v in ck.items()}
    missing, unexpected = load_pretrained_det(m, {"model": ck})
    assert all(torch.equal(ck[k], before[k]) for k in before) and set(ck) == set(before)            # the caller's dict is left alone
    assert unexpected == ["image_adapter.rel_pos_table_list.0.weight"]
    assert set(missing) == set(D.BUCKETS) | {"encoder.layers.%d.self_attn.rel_pos_%s" % (i, a) for i in (0, 1) for a in "hw"}
    assert torch.equal(m.image_adapter.rel_pos_table.weight, ck["image_adapter.rel_pos_table_list.0.weight"])
    pos = m.image_adapter.pos_embed
    assert tuple(pos.shape) == (32 * 32 + 1, dim) and torch.equal(pos[0], ck["image_adapter.pos_embed"][0])
    want = torch.nn.functional.interpolate(ck["image_adapter.pos_embed"][1:].reshape(1, 16, 16, dim).permute(0, 3, 1, 2), size=(32, 32),
                                           mode="bicubic", align_corners=False).permute(0, 2, 3, 1).reshape(-1, dim)
    assert torch.allclose(pos[1:], want)
    assert torch.equal(m.encoder.layers[1].image_ffn[3].weight, ck["encoder.layers.1.image_ffn.3.weight"])
    bias, bias_w = m.image_adapter.get_rel_pos_bias(), m.image_adapter.get_rel_pos_bias(True)   # 31 -> 63 bicubic; 31 -> 31 as it is
    assert tuple(bias.shape) == (fx["args"]["attention_heads"], 1024, 1024) and tuple(bias_w.shape) == (fx["args"]["attention_heads"], 256, 256)
    assert torch.equal(bias_w[0, 17, 0], m.image_adapter.rel_pos_table.weight[(1 + 15) * 31 + (1 + 15), 0])


def test_lr_decay_rate_on_the_names_of_the_references_docstring():
    from one_peace_amd.one_peace_vision import get_onepeace_lr_decay_rate as rate
    assert rate("backbone.net.image_adapter.pos_embed", 0.9, 40) == 0.9 ** 41
    assert rate("backbone.net.encoder.layers.0.gamma_1", 0.9, 40) == 0.9 ** 40
    assert rate("backbone.net.encoder.layers.39.self_attn.q_proj.weight", 0.9, 40) == 0.9 ** 1
    assert rate("backbone.net.encoder.layers.3.residual.weight", 0.9, 40) == 1.0
    assert rate("backbone.simfp_2.0.weight", 0.9, 40) == 1.0
    assert rate("roi_heads.box_head.layers.2.weight", 0.9, 40) == 1.0                 # not the backbone: no decay
    assert rate("backbone.net.encoder.layers.11.image_ffn.3.bias", 0.8, 12) == 0.8 ** 1


def test_rp_bias_is_refused():
    from one_peace_amd.one_peace_vision import OnePeaceDetViT
    with pytest.raises(NotImplementedError):
        OnePeaceDetViT(**dict(D.fixture()["args"], rp_bias=True))
    with pytest.raises(NotImplementedError):
        OnePeaceDetViT(**dict(D.fixture()["args"], pretrained="x.pkl"))


def test_checkpointed_and_padded_grids_run_the_same_statement():
    """use_checkpoint gives the same numbers; a window size that does not divide the grid pads as detectron2 does (the padded keys'
    v = v_proj.bias matters: the result differs from a zero pad row)."""
    from one_peace_amd import ops
    fx = D.fixture()
    a, b = D.build(fx), D.build(fx, use_checkpoint=True)
    x = D.image(fx).float()
    oa = a(x)["last_feat"]
    ob = b(x)["last_feat"]
    assert torch.equal(oa, ob)
    (ob * D.cotangent(fx).float()).sum().backward()
    assert all(p.grad is not None for p in b.parameters())
    torch.manual_seed(0)
    qkv = torch.randn(20 * 24, 3 * 64)
    pad = torch.randn(3 * 64)
    assert not torch.allclose(ops.window_attention(qkv, None, None, None, 1, 20, 24, 1, 16, pad_row=pad),
                              ops.window_attention(qkv, None, None, None, 1, 20, 24, 1, 16))
