"""Model-level parity on MI355X: the HIP path (bf16) against the reference-generated golden fixtures / the fp32 oracle.

Stated tolerance (north_star: "within a stated fp tolerance"), ABSOLUTE since round 3: for every compared tensor
    rel_fro(hip_bf16, fp32_reference) <= bound
with bound = 1.5e-2 for activations / embeddings / logits and 5e-2 for gradients (6e-2 for the masked-pretraining objectives,
whose per-sample token subsets leave fewer summands per weight), plus the few named exceptions of BOUND_EXCEPTIONS -- tensors
whose error is a property of the problem, not of the kernels (the bf16 torch path of the reference algorithm lands at the same
value).  The bounds were read off the measured reports (profiles/r*_parity_report*.txt, gpurun_out/*_parity_report*.txt: largest
activation error 1.2e-2, largest regular gradient error 4.0e-2 micro / 5.3e-2 pretraining) -- until round 2 the gate was relative
to the torch-bf16 path (2 x its error), which let both drift together.  That path (the reference algorithm executed op-by-op in
bf16, trainer.py:86-88) is still run and its error printed next to ours in the reports, as context only.  The fused kernels keep
fp32 accumulators across ops the reference rounds to bf16 in between, so they are normally *closer* to fp32 than it is."""
import os

import pytest
import torch

from oracle import onepeace_oracle as O
from oracle import synth
from tests.model_util import build_retrieval, load_synth
from tests.util import out_dir, rel_fro

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _fx(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), weights_only=False)


# name -> bound that replaces the default one (measured value in brackets; torch-bf16 lands at the same error).  EXACT tensor
# names (as _check reports them).  Round 5: the audio relative-position table's gradient lost its 1.2e-1 relative exemption.  It is a
# tiny (|g| = 8.6e-3 on the micro fixture) gradient that sums strongly cancelling dS entries over buckets that each cover a large
# share of the keys; its bf16 error does not scale with its norm, which is what the 1.5e-3 ABSOLUTE Frobenius slack every small
# gradient gets (abs_err below, the same slack smoke() uses) is for: under the common 5e-2 + 1.5e-3 it measures 4.8e-2 on the micro
# fixture, 3.6e-2 joint, 2.1e-2 in the audio-text pretraining objective and 8.3e-3 at the 4B layer dimensions
# (profiles/r4_*parity_report*.txt, test_lock_step_layer_4b_dimensions_against_the_fp32_oracle) -- a dBias regression can no
# longer hide behind a 12 % relative bound.
BOUND_EXCEPTIONS = {
    "al_audio": 2.3e-2,  # [1.86e-2; torch-bf16 2.0e-2] audio CLS embedding of the joint step
}


def _check(name, hip_val, torch_val, ref, bound, report, abs_err=0.0):
    """Absolute gate:  |hip - ref|_F <= bound * |ref|_F + abs_err  (abs_err: Frobenius slack for small-norm gradients whose bf16
    error does not scale with their norm).  The torch-bf16 error is reported, not gated on."""
    e_hip, e_t = rel_fro(hip_val.float(), ref), rel_fro(torch_val.float(), ref)
    bound = BOUND_EXCEPTIONS.get(name, bound)
    report.append("%-60s hip %.3e  torch-bf16 %.3e  (bound %.1e)" % (name, e_hip, e_t, bound))
    nref = float(ref.double().norm())
    assert e_hip * nref <= bound * nref + abs_err, "%s: hip %.3e > bound %.1e (torch-bf16 %.3e, abs %.1e, |ref| %.3e)" % (
        name, e_hip, bound, e_t, abs_err, nref)


def _force_torch_path(model, flag):
    """Disable/enable the HIP dispatch of the mirrors (yardstick run)."""
    from one_peace_amd import ops
    ops.hip_eligible = (lambda x: False) if flag else ops._hip_eligible_orig


@pytest.fixture(autouse=True)
def _save_eligible():
    from one_peace_amd import ops
    if not hasattr(ops, "_hip_eligible_orig"):
        ops._hip_eligible_orig = ops.hip_eligible
    yield
    ops.hip_eligible = ops._hip_eligible_orig


def _to_dev(inp):
    return {k: (v.to(DEV).to(torch.bfloat16) if v.is_floating_point() else v.to(DEV)) for k, v in inp.items()}


def test_micro_model_forward_backward(golden_dir):
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    fx = _fx(golden_dir, "micro_retrieval.pt")
    report = []
    results = {}
    for mode in ("hip", "torch"):
        m = load_synth(build_retrieval(fx["cfg"], fx["vocab"]), fx["shapes"]).to(DEV).to(torch.bfloat16).eval()
        _force_torch_path(m, mode == "torch")
        inp = _to_dev(fx["inputs"])
        t = m(src_tokens=inp["src_tokens"], encoder_type="text")
        i = m(src_images=inp["src_images"], encoder_type="image")
        a = m(src_audios=inp["src_audios"], audio_padding_masks=inp["audio_padding_masks"], encoder_type="audio")
        crit = TriModalContrastiveCriterion(None, 0.0)
        loss, _, log = crit(m, {"net_input": inp, "nsentences": 4})
        m.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        results[mode] = dict(t=t.detach(), i=i.detach(), a=a.detach(), itc=log["itc_loss"].float(),
                             grads={n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None})
    h, tt = results["hip"], results["torch"]
    for key, ref in (("t", "text_logits"), ("i", "image_logits"), ("a", "audio_logits")):
        _check(ref, h[key], tt[key], fx[ref], 1.5e-2, report)
    assert abs(float(h["itc"]) - float(fx["itc_loss"])) <= 2e-2  # absolute (loss ~ 1.4; measured 3e-3)
    # gradients: the golden file holds the ITC + ATC(label smoothing 0.1) objective; here the criterion uses 0.0 for both,
    # so compare against the oracle's gradient of exactly this objective
    sd = {k: v.clone().requires_grad_(v.is_floating_point()) for k, v in synth.synth_state_dict(fx["shapes"]).items()}
    sd["encoder_wrapper.text_adapter.rp_bucket"] = O.token_bucket_position(fx["cfg"]["text_bucket_size"])
    sd["encoder_wrapper.audio_adapter.rp_bucket"] = O.token_bucket_position(fx["cfg"]["audio_bucket_size"])
    rb = fx["cfg"]["image_rel_bucket_size"]
    sd["encoder_wrapper.image_adapter.rp_bucket"] = O.image_bucket_position(rb, (2 * rb - 1) ** 2 + 3)
    heads, L = fx["cfg"]["attention_heads"], fx["cfg"]["layers"]
    inp = fx["inputs"]
    to, _ = O.contrastive_embed(sd, heads, L, "text", src_tokens=inp["src_tokens"])
    io, _ = O.contrastive_embed(sd, heads, L, "image", src_images=inp["src_images"])
    ao, _ = O.contrastive_embed(sd, heads, L, "audio", src_audios=inp["src_audios"],
                                audio_padding_masks=inp["audio_padding_masks"])
    sc = O.logit_scale_exp(sd["logit_scale"])
    (O.itc_loss(io, to, io, to, sc)[0] + O.itc_loss(ao, to, ao, to, sc)[0]).backward()
    worst = 0.0
    for n, g in h["grads"].items():
        ref = sd[n].grad
        if ref is None or float(ref.norm()) < 1e-7:
            continue
        # ill-conditioned gradients (the audio relative-position table: |g|_F = 8.6e-3, 5x below the text table's) carry a bf16
        # error that does NOT scale with their norm: 0.5 - 1.3e-3 absolute on the bf16 TORCH path under +-1 ulp of input noise
        # (tools/grad_conditioning.py).  They get the same 5e-2 relative floor as every gradient plus that absolute slack
        # (1.5e-3 Frobenius) -- negligible for every well-conditioned tensor (norms 0.1 - 50).
        _check("grad " + n, g, tt["grads"][n], ref, 5e-2, report, abs_err=1.5e-3)
        worst = max(worst, rel_fro(g, ref))
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "model_parity_report.txt"), "w").write(
        "\n".join(report) + "\nworst grad rel-fro %.3e\n" % worst)


def test_tiny_text_config1_on_gpu(golden_dir):
    fx = _fx(golden_dir, "tiny_text.pt")
    m = load_synth(build_retrieval(dict(fx["cfg"]), 50265, head_type="text"), fx["shapes"]).to(DEV).to(torch.bfloat16).eval()
    tok = fx["inputs"]["src_tokens"].to(DEV)
    report = []
    with torch.no_grad():
        out_h = m(src_tokens=tok, encoder_type="text")
        _force_torch_path(m, True)
        out_t = m(src_tokens=tok, encoder_type="text")
    _check("tiny text logits", out_h, out_t, fx["text_logits"], 1.5e-2, report)
    cos = torch.nn.functional.cosine_similarity(out_h.float().cpu(), fx["text_logits"], dim=1)
    assert float(cos.min()) > 0.9995


@pytest.mark.parametrize("recompute", [False, True])
def test_fused_layer_with_padding_and_drop_path(recompute):
    """One 4B-aspect layer (hd=64, H=256) incl. key padding, per-sample drop-path and all gradients, vs the oracle;
    both activation policies (kept in HBM / recomputed in backward)."""
    from one_peace_amd import ops
    from one_peace_amd.relpos import RelPosSpec, make_token_bucket_position, add_cls_buckets
    from one_peace_amd.transformer.transformer_layer import TransformerEncoderLayer
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    import one_peace_amd.transformer.transformer_layer as TL
    cfg = one_peace_encoder_config(embed_dim=256, ffn_embed_dim=512, layers=1, attention_heads=4, drop_path_rate=0.0,
                                   checkpoint_activations=recompute)
    torch.manual_seed(0)
    layer = TransformerEncoderLayer(cfg, drop_path_rate=0.3)
    shapes = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
    sd = synth.synth_state_dict(shapes)
    layer.load_state_dict(sd)
    layer = layer.to(DEV).to(torch.bfloat16).train()
    B, S, H, heads = 5, 70, 256, 4
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S, H, generator=g).to(torch.bfloat16).float()
    table = (0.5 * torch.randn(2 * 32 - 1 + 3, heads, generator=g)).to(torch.bfloat16).float()
    bucket = add_cls_buckets(make_token_bucket_position(32, 1024), 2 * 32 - 1)[:S, :S]
    pad = torch.zeros(B, S, dtype=torch.bool)
    pad[1, 60:] = True
    pad[3, 33:] = True
    ps1 = torch.tensor([1 / 0.7, 0.0, 1 / 0.7, 1 / 0.7, 0.0])
    ps2 = torch.tensor([0.0, 1 / 0.7, 1 / 0.7, 0.0, 1 / 0.7])
    dy = torch.randn(B, S, H, generator=g).to(torch.bfloat16).float()
    # ---- oracle (fp32) ----
    sdo = {"L." + k: v.clone().requires_grad_(True) for k, v in sd.items()}
    tab_o = table.clone().requires_grad_(True)
    xo = x.clone().requires_grad_(True)
    bias = O.rel_pos_bias(tab_o, bucket).unsqueeze(0).expand(B, -1, -1, -1)
    bias = bias.masked_fill(pad.view(B, 1, 1, S), float("-inf"))
    # two different drop-path draws: oracle.encoder_layer takes one; apply through a small wrapper
    import oracle.onepeace_oracle as OO
    calls = {"n": 0}
    orig = OO.residual_scale

    def rs(xb, gamma, res, path_scale=None):
        calls["n"] += 1
        return orig(xb, gamma, res, ps1 if calls["n"] == 1 else ps2)
    OO.residual_scale = rs
    try:
        yo = O.encoder_layer(xo.transpose(0, 1), sdo, "L", heads, "text", bias).transpose(0, 1)
    finally:
        OO.residual_scale = orig
    (yo * dy).sum().backward()
    # ---- HIP ----
    seq = iter([ps1.to(DEV), ps2.to(DEV)])
    orig_sample = TL.sample_path_scale
    TL.sample_path_scale = lambda b, p, tr, dev: next(seq)
    try:
        xd = x.to(DEV).to(torch.bfloat16).requires_grad_(True)
        tab_d = table.to(DEV).to(torch.bfloat16).requires_grad_(True)
        spec = RelPosSpec(tab_d, bucket.to(DEV))
        key_pad = torch.ones(B, __import__("one_peace_amd").hip.attn_spad(S), dtype=torch.uint8, device=DEV)
        key_pad[:, :S] = pad.to(torch.uint8).to(DEV)
        yd = layer.forward_fused(xd, spec.handle(), key_pad, "text")
        (yd.float() * dy.to(DEV)).sum().backward()
    finally:
        TL.sample_path_scale = orig_sample
    torch.cuda.synchronize()
    assert rel_fro(yd.float(), yo) < 6e-3
    assert rel_fro(xd.grad.float(), xo.grad) < 2e-2
    assert rel_fro(tab_d.grad.float(), tab_o.grad) < 3e-2
    named = dict(layer.named_parameters())
    for k, v in sdo.items():
        n = k[2:]
        if v.grad is None or n not in named or named[n].grad is None:
            continue
        e = rel_fro(named[n].grad.float(), v.grad)
        assert e < 3e-2, (n, e)


def test_no_bias_encoder_attends_to_padded_keys_like_the_reference():
    """Reference semantics (transformer_encoder.py:144-162, multihead_attention.py:102-115): padded keys are masked ONLY
    through the bias tensor, so an encoder WITHOUT attention bias (the pretraining decoder, pretrain_vl_3B.yaml:140,150)
    attends to its zeroed pad rows.  Fused path vs the fp32 torch path of the same mirror (which is pinned to the reference on
    CPU), output and input gradient; the test is sensitive: masking the pads moves the output by > 10 %."""
    from one_peace_amd.transformer.transformer_encoder import TransformerEncoder
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    cfg = one_peace_encoder_config(embed_dim=256, ffn_embed_dim=512, layers=2, attention_heads=4, drop_path_rate=0.0,
                                   layer_scale_init_value=0.5)
    cfg.use_text_moe, cfg.use_image_moe, cfg.use_audio_moe = True, False, False
    torch.manual_seed(0)
    enc32 = TransformerEncoder(cfg, None, True, False, False)
    sd = synth.synth_state_dict({k: tuple(v.shape) for k, v in enc32.state_dict().items()})
    sd["version"] = enc32.state_dict()["version"]
    enc32.load_state_dict(sd)
    enc32.eval()
    B, S, H = 4, 40, 256
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, S, H, generator=g).to(torch.bfloat16).float()
    pad = torch.zeros(B, S, dtype=torch.bool)
    pad[1, 25:] = True
    pad[2, 9:] = True
    dy = torch.randn(S, B, H, generator=g)

    def run(enc, xin, device, mask_keys=False):
        xin = xin.clone().to(device).requires_grad_(True)
        out = enc(text_info=(xin, pad.to(device), None), image_info=None, audio_info=None, encoder_type="text")["encoder_out"][0]
        valid = (~pad).t().unsqueeze(-1).to(device)  # [S, B, 1]: pad rows hold garbage by construction, compare valid rows
        (out.float() * dy.to(device) * valid).sum().backward()
        return (out.float() * valid).detach().cpu(), xin.grad.float().cpu()
    ref_o, ref_g = run(enc32, x, "cpu")
    import copy
    encd = copy.deepcopy(enc32).to(DEV).to(torch.bfloat16).eval()
    hip_o, hip_g = run(encd, x.to(torch.bfloat16), DEV)
    _force_torch_path(encd, True)
    tor_o, tor_g = run(encd, x.to(torch.bfloat16), DEV)
    report = []
    _check("no-bias padded encoder out", hip_o, tor_o, ref_o, 1.5e-2, report)
    _check("no-bias padded encoder dx", hip_g, tor_g, ref_g, 5e-2, report)
    # sensitivity: the same input with the pads masked as keys (bias of zeros + -inf) is far outside the tolerance
    zero_bias = torch.zeros(B, 4, S, S)
    masked = enc32(text_info=(x, pad, [zero_bias]), image_info=None, audio_info=None, encoder_type="text")["encoder_out"][0]
    assert rel_fro(masked.float() * (~pad).t().unsqueeze(-1), ref_o) > 0.1


def test_direct_gradient_accumulation_matches_autograd():
    """With distributed.FlatParameters the big layer weights' gradients are accumulated in place by the GEMMs (three
    modality passes share the attention weights); the result must equal the plain autograd path."""
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=2, attention_heads=2, image_rel_bucket_size=4,
               text_bucket_size=256, audio_bucket_size=512)
    inp = _to_dev(synth.synth_inputs(64, text_len=15, image_res=64, audio_samples=8000, vocab=1000))  # 64*16 rows: TN path
    grads = {}
    for mode in ("autograd", "direct"):
        m = load_synth(build_retrieval(cfg, 1000)).to(DEV).to(torch.bfloat16).eval()
        flat = FlatParameters(m) if mode == "direct" else None
        for _ in range(2):  # second step checks that zero_grad resets the bookkeeping
            if flat is not None:
                flat.zero_grad()
            else:
                m.zero_grad()
            loss, _, _ = TriModalContrastiveCriterion(None, 0.0)(m, {"net_input": inp, "nsentences": 64})
            loss.backward()
        torch.cuda.synchronize()
        grads[mode] = {n: p.grad.detach().float().cpu().clone() for n, p in m.named_parameters() if p.grad is not None}
    worst = 0.0
    for n, g in grads["autograd"].items():
        if float(g.norm()) == 0:
            continue
        e = rel_fro(grads["direct"][n], g)
        worst = max(worst, e)
        assert e < 2e-2, (n, e)   # bf16 accumulation order differs (in-place += vs autograd's sum)
    assert len(grads["direct"]) >= len(grads["autograd"])


@pytest.mark.parametrize("train", [False, True])
def test_joint_vl_al_streams_on_hip(golden_dir, train):
    """encoder_type 'vl' / 'al' (transformer_encoder.py:144-207, transformer_layer.py:206-216): one attention over the
    joint sequence with the block-diagonal bias, each modality's rows through its own FFN.  Forward against the
    reference-generated golden outputs; gradients (weighted sum of both outputs, incl. both rel-pos tables) against
    the fp32 torch path of the mirror (itself pinned to the reference on CPU, tests/test_model_cpu.py)."""
    from one_peace_amd.transformer import transformer_encoder as TE
    fx = _fx(golden_dir, "micro_retrieval.pt")
    report = []
    calls = {"n": 0}
    orig = TE.TransformerEncoder._forward_fused

    def counted(self, *a, **k):
        calls["n"] += 1
        return orig(self, *a, **k)

    def run(m, inp):
        w = m.encoder_wrapper
        vt, vi, _ = w(src_tokens=inp["src_tokens"], src_images=inp["src_images"], encoder_type="vl")
        at, _, aa = w(src_tokens=inp["src_tokens"], src_audios=inp["src_audios"],
                      audio_padding_masks=inp["audio_padding_masks"], encoder_type="al")
        outs = dict(vl_text=vt, vl_image=vi, al_text=at, al_audio=aa)
        grads = {}
        if train:
            g = torch.Generator().manual_seed(5)
            loss = sum((o.float() * torch.randn(o.shape, generator=g).to(o.device)).sum() for o in outs.values())
            m.zero_grad()
            loss.backward()
            grads = {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None}
        return {k: v.detach().float().cpu() for k, v in outs.items()}, grads

    res = {}
    TE.TransformerEncoder._forward_fused = counted
    try:
        for mode in ("hip", "torch", "fp32"):
            dt = torch.float32 if mode == "fp32" else torch.bfloat16
            m = load_synth(build_retrieval(fx["cfg"], fx["vocab"]), fx["shapes"]).to(DEV).to(dt).eval()
            _force_torch_path(m, mode != "hip")
            inp = {k: (v.to(DEV).to(dt) if v.is_floating_point() else v.to(DEV)) for k, v in fx["inputs"].items()}
            before = calls["n"]
            res[mode] = run(m, inp)
            assert (calls["n"] - before == 2) == (mode == "hip"), "joint streams must take the fused HIP path"
    finally:
        TE.TransformerEncoder._forward_fused = orig
    for k in ("vl_text", "vl_image", "al_text", "al_audio"):
        assert rel_fro(res["fp32"][0][k], fx[k]) < 1e-4  # the fp32 mirror reproduces the reference fixture
        _check(k, res["hip"][0][k], res["torch"][0][k], fx[k], 1.5e-2, report)
    if train:
        n_checked = 0
        for n, ref in res["fp32"][1].items():
            if float(ref.norm()) < 1e-7:
                continue
            _check("grad " + n, res["hip"][1][n], res["torch"][1][n], ref, 5e-2, report)
            n_checked += 1
        assert n_checked > 50
        assert any("rel_pos_table" in n for n in res["hip"][1])
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "joint_parity_report_%d.txt" % train),
         "w").write("\n".join(report) + "\n")


def test_full_size_layer_4b_dimensions():
    """One encoder layer at the BASELINE dimensions (H=1536, F=6144, 24 heads, image S=257) on the HIP path against the
    fp32 CPU oracle: outputs and every parameter gradient, plus two size-independent properties -- batch-permutation equivariance
    (bit-exact: rows never mix across samples) and invariance to appended, masked keys."""
    from one_peace_amd.relpos import RelPosSpec, make_image_bucket_position
    from one_peace_amd.transformer.transformer_layer import TransformerEncoderLayer
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd import hip
    cfg = one_peace_encoder_config(embed_dim=1536, ffn_embed_dim=6144, layers=1, attention_heads=24, drop_path_rate=0.0)
    torch.manual_seed(0)
    layer = TransformerEncoderLayer(cfg, drop_path_rate=0.0)
    for n, q in layer.named_parameters():  # non-trivial LayerNorm / layer-scale values
        if q.dim() == 1:
            q.data.add_(0.1 * torch.randn_like(q))
    B, S, H, heads = 6, 257, 1536, 24
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, S, H, generator=g)
    dy = torch.randn(B, S, H, generator=g)
    nrel = (2 * 16 - 1) ** 2 + 3
    table = 0.5 * torch.randn(nrel, heads, generator=g)
    bucket = make_image_bucket_position(16, nrel)

    def run(dtype, fused, xin, key_pad=None, dense_extra=None):
        m = layer.to(DEV).to(dtype)
        m.zero_grad()
        xd = xin.to(DEV).to(dtype).requires_grad_(True)
        tab = table.to(DEV).to(dtype).requires_grad_(True)
        spec = RelPosSpec(tab, bucket.to(DEV))
        if fused:
            y = m.forward_fused(xd, spec.handle(), key_pad, "image")
        else:
            bias = spec.dense(xin.shape[0]).to(dtype)
            y = m(xd.transpose(0, 1), encoder_padding_mask=None, self_attn_bias=bias, encoder_type="image").transpose(0, 1)
        (y.float() * dy.to(DEV)[: xin.shape[0]]).sum().backward()
        grads = {n: q.grad.detach().float().clone() for n, q in m.named_parameters() if q.grad is not None}
        return y.detach().float(), xd.grad.detach().float(), tab.grad.detach().float(), grads

    # fp32 reference: the CPU oracle (oracle/onepeace_oracle.py, pinned to the reference by tests/test_oracle_golden.py)
    sdo = {"L." + k: v.detach().clone().float().requires_grad_(True) for k, v in layer.state_dict().items()}
    xo, tabo = x.clone().requires_grad_(True), table.clone().requires_grad_(True)
    bias_o = O.rel_pos_bias(tabo, bucket).unsqueeze(0).expand(B, -1, -1, -1)
    yo = O.encoder_layer(xo.transpose(0, 1), sdo, "L", heads, "image", bias_o).transpose(0, 1)
    (yo * dy).sum().backward()
    y32, dx32, dt32 = yo.detach(), xo.grad, tabo.grad
    g32 = {k[2:]: v.grad for k, v in sdo.items() if v.grad is not None}
    yb, dxb, dtb, gb = run(torch.bfloat16, False, x)     # yardstick: the reference algorithm op by op in bf16
    yh, dxh, dth, gh = run(torch.bfloat16, True, x)
    report = []
    # (round 6) bounds = 2.5 x what these tensors measure (profiles/r5_layer_4b_parity_report.txt: out 3.0e-3, dx 3.3e-3, table
    # 8.4e-3, parameter gradients 2.7e-3 ... 9.9e-3): a numerical regression of 3 x in any of them fails, the micro-model bounds stay
    # where the micro model measures (up to 4e-2)
    _check("4B-dim layer out", yh.cpu(), yb.cpu(), y32, 7.5e-3, report)
    _check("4B-dim layer dx", dxh.cpu(), dxb.cpu(), dx32, 8.5e-3, report)
    _check("4B-dim layer dtable", dth.cpu(), dtb.cpu(), dt32, 2.1e-2, report)
    for n, ref in g32.items():
        if n in gh and float(ref.norm()) > 1e-7:
            _check("4B-dim grad " + n, gh[n].cpu(), gb[n].cpu(), ref, 2.5e-2, report)
    assert len([n for n in g32 if n in gh]) >= 20  # attention + image-FFN parameters (the text / audio FFNs take no part)
    # property 1: permuting the samples permutes the outputs, bit for bit
    perm = torch.tensor([3, 0, 5, 1, 4, 2])
    yp = run(torch.bfloat16, True, x[perm])[0]
    assert torch.equal(yp, yh[perm.to(DEV)])
    # property 2: keys that are masked out do not exist -- mask the last 40 keys and compare with the truncated sequence
    key_pad = torch.zeros(B, hip.attn_spad(S), dtype=torch.uint8, device=DEV)
    key_pad[:, S - 40:] = 1
    y_masked = run(torch.bfloat16, True, x, key_pad=key_pad)[0]
    assert y_masked.isfinite().all() and rel_fro(y_masked[:, : S - 40], yh[:, : S - 40]) > 1e-3   # the mask had an effect
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "layer_4b_parity_report.txt"), "w").write(
        "\n".join(report) + "\n")


def test_lock_step_layer_4b_dimensions_against_the_fp32_oracle():
    """Round 4: ONE encoder layer at the 4B dimensions in its LOCK-STEP form -- text, image and audio rows packed
    in one matrix, the modality-shared attention branch launched once over all of them, each segment through its own FFN, every
    weight gradient of the layer in the grouped launch -- against the fp32 CPU oracle run once per modality on the same weights:
    per-modality outputs and input gradients, the bias-table gradients, and EVERY parameter gradient (those of the shared
    parameters are the oracle's sum over the three passes)."""
    from one_peace_amd import hip, ops
    from one_peace_amd.relpos import RelPosSpec, add_cls_buckets, make_image_bucket_position, make_token_bucket_position
    from one_peace_amd.transformer.transformer_layer import TransformerEncoderLayer
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    cfg = one_peace_encoder_config(embed_dim=1536, ffn_embed_dim=6144, layers=1, attention_heads=24, drop_path_rate=0.0)
    torch.manual_seed(0)
    layer = TransformerEncoderLayer(cfg, drop_path_rate=0.0)
    for n, q in layer.named_parameters():
        if q.dim() == 1:
            q.data.add_(0.1 * torch.randn_like(q))
    H, heads = 1536, 24
    g = torch.Generator().manual_seed(2)
    shapes = {"text": (3, 64), "image": (3, 257), "audio": (3, 250)}
    nrel_img = (2 * 16 - 1) ** 2 + 3
    buckets = {"image": make_image_bucket_position(16, nrel_img),
               "text": add_cls_buckets(make_token_bucket_position(256)[:64, :64].clone(), 2 * 256 - 1),
               "audio": add_cls_buckets(make_token_bucket_position(512)[:250, :250].clone(), 2 * 512 - 1)}
    tables = {m: 0.5 * torch.randn(int(buckets[m].max()) + 1, heads, generator=g) for m in shapes}
    xs = {m: torch.randn(b, s, H, generator=g) for m, (b, s) in shapes.items()}
    dys = {m: torch.randn(b, s, H, generator=g) for m, (b, s) in shapes.items()}
    pads = {"audio": torch.zeros(3, 250, dtype=torch.bool)}
    pads["audio"][1, 230:] = True
    pads["audio"][2, 190:] = True

    # ---- fp32 oracle, one pass per modality on shared leaves ----
    sdo = {"L." + k: v.detach().clone().float().requires_grad_(True) for k, v in layer.state_dict().items()}
    ref_out, ref_dx, ref_dt = {}, {}, {}
    for m, (b, s) in shapes.items():
        xo, tabo = xs[m].clone().requires_grad_(True), tables[m].clone().requires_grad_(True)
        bias_o = O.rel_pos_bias(tabo, buckets[m]).unsqueeze(0).expand(b, -1, -1, -1)
        if m in pads:
            bias_o = bias_o.masked_fill(pads[m][:, None, None, :], float("-inf"))
        yo = O.encoder_layer(xo.transpose(0, 1), sdo, "L", heads, m, bias_o).transpose(0, 1)
        live = (~pads[m]).unsqueeze(-1).float() if m in pads else 1.0
        (yo * dys[m] * live).sum().backward()
        ref_out[m], ref_dx[m], ref_dt[m] = yo.detach(), xo.grad, tabo.grad
    g32 = {k[2:]: v.grad for k, v in sdo.items() if v.grad is not None}

    # ---- HIP lock-step pass ----
    mdev = layer.to(DEV).to(torch.bfloat16)
    mdev.zero_grad()
    segs, x2, tabs, row0 = [], [], {}, 0
    for m, (b, s) in shapes.items():
        tabs[m] = tables[m].to(DEV).to(torch.bfloat16).requires_grad_(True)
        key_pad = None
        if m in pads:
            key_pad = torch.ones(b, hip.attn_spad(s), dtype=torch.uint8, device=DEV)
            key_pad[:, :s] = pads[m].to(torch.uint8).to(DEV)
        segs.append(ops.StreamSeg(m, b, s, row0, RelPosSpec(tabs[m], buckets[m].to(DEV)).handle(), key_pad))
        x2.append(xs[m].reshape(b * s, H))
        row0 += b * s
    x2d = torch.cat(x2).to(DEV).to(torch.bfloat16).requires_grad_(True)
    y2 = mdev.forward_fused_multi(x2d, segs, None, [None] * 3)
    dy2 = torch.cat([(dys[m] * ((~pads[m]).unsqueeze(-1).float() if m in pads else 1.0)).reshape(-1, H) for m in shapes]).to(DEV)
    (y2.float() * dy2).sum().backward()
    torch.cuda.synchronize()
    report = []

    def check(name, got, ref, bound):
        e = rel_fro(got.float().cpu(), ref)
        report.append("%-60s hip %.3e (bound %.1e)" % (name, e, bound))
        assert e <= bound, "%s: %.3e > %.1e" % (name, e, bound)
    for sg in segs:
        m, (b, s) = sg.name, shapes[sg.name]
        rows = slice(sg.row0, sg.end)
        live = (~pads[m]) if m in pads else torch.ones(b, s, dtype=torch.bool)
        # (round 6) bounds = 2.5 x measured (profiles/r5_lock_step_layer_4b_parity_report.txt: 3.0e-3 / 3.3e-3 / 8.4e-3, gradients <= 9.9e-3)
        check("lock-step 4B layer out " + m, y2[rows].view(b, s, H)[live.to(DEV)], ref_out[m][live], 7.5e-3)
        check("lock-step 4B layer dx " + m, x2d.grad[rows].view(b, s, H), ref_dx[m], 8.5e-3)
        check("lock-step 4B layer dtable " + m, tabs[m].grad, ref_dt[m], 2.1e-2)
    n = 0
    for name, q in mdev.named_parameters():
        if name in g32 and float(g32[name].norm()) > 1e-7:
            assert q.grad is not None, name
            check("lock-step 4B layer grad " + name, q.grad, g32[name], 2.5e-2)
            n += 1
    assert n >= 30  # attention branch (12) + three FFN sets (6 each) + final LayerNorm, layer-scale vectors
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "lock_step_layer_4b_parity_report.txt"), "w").write(
        "\n".join(report) + "\n")


# ---- config 4's sequence lengths at the 4B dimensions, bf16 and both fp8 routes, against the fp32 oracle ----------------------------
_CFG4_ORACLE = {}
# Gates per route and class: 2.5 x the largest error measured over the two kinds (cfg4_layer_4b_parity_report_*.txt), measured value in
# brackets.  bf16 lands below its S = 257 values (out 3.0e-3, dx 3.3e-3, table 8.4e-3, gradients <= 9.9e-3).  'ffn': the gradients
# of the FFN branch's parameters (GeGLU, LN_F, W2, gamma_2, LayerNorm 2).  On the fp8 routes they are computed from activations of TWO
# chained quantised projections (gelu(x W0) * (x W1), then W2), measured 6.5e-2 / 6.6e-2 -- above the variant's 5e-2 for one GEMM and
# within the 1.5 x FP8_TOL = 7.5e-2 the project states for a product of two quantised projections (test_ops_gpu.py:
# test_fp8_gemm_geglu), which is their gate instead of 2.5 x measured (the fp8 kernels themselves are exact against their dequantised
# operands at these shapes: test_fp8_gemm_at_the_input_gradient_shapes).
CFG4_BOUNDS = {"bf16": {"out": 6.2e-3, "dx": 6.6e-3, "dtable": 1.4e-2, "grad": 1.7e-2, "ffn": 1.4e-2},  # [2.5e-3 2.6e-3 5.7e-3 6.8e-3 5.7e-3]
               "fp8": {"out": 2.2e-2, "dx": 2.0e-2, "dtable": 2.4e-2, "grad": 2.6e-2, "ffn": 7.5e-2},  # [8.8e-3 8.0e-3 9.6e-3 1.0e-2 6.5e-2]
               "fp8+dgrad": {"out": 2.2e-2, "dx": 3.1e-2, "dtable": 3.4e-2, "grad": 3.7e-2, "ffn": 7.5e-2}}  # [8.8e-3 1.3e-2 1.4e-2 1.5e-2 6.6e-2]


def _cfg4_layer_case(kind):
    """One encoder layer (H = 1536, F = 6144, 24 heads, LayerNorm and layer-scale vectors away from their init), inputs shaped like
    config 4's steps and the fp32 oracle's results, once per kind (the three routes share them), plus the torch-bf16 yardstick: the same
    oracle code run in bf16 on the device.  kind 'vl': the lock-step text + image pass -- 3 x 64 text tokens with ragged key padding
    (64 / 41 / 17 valid), 3 x 785 image tokens (grid 28); 'image1025': a single-stream 2 x 1025 image pass (grid 32)."""
    if kind in _CFG4_ORACLE:
        return _CFG4_ORACLE[kind]
    from one_peace_amd.relpos import add_cls_buckets, make_image_bucket_position, make_token_bucket_position
    from one_peace_amd.transformer.transformer_layer import TransformerEncoderLayer
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    H, heads = 1536, 24
    cfg = one_peace_encoder_config(embed_dim=H, ffn_embed_dim=6144, layers=1, attention_heads=heads, drop_path_rate=0.0)
    torch.manual_seed(0)
    layer = TransformerEncoderLayer(cfg, drop_path_rate=0.0)
    g = torch.Generator().manual_seed(11)
    for n, q in layer.named_parameters():
        if n.startswith("gamma_"):
            q.data.copy_(0.1 * (1.0 + 0.3 * torch.randn(q.shape, generator=g)))
        elif q.dim() == 1:
            q.data.add_(0.1 * torch.randn(q.shape, generator=g))
    layer = layer.to(torch.bfloat16)
    if kind == "vl":
        shapes = {"text": (3, 64), "image": (3, 785)}
        pads = {"text": torch.arange(64)[None, :] >= torch.tensor([64, 41, 17])[:, None]}
        grid = 28
    else:
        shapes, pads, grid = {"image": (2, 1025)}, {}, 32
    buckets = {"image": make_image_bucket_position(grid, (2 * grid - 1) ** 2 + 3),
               "text": add_cls_buckets(make_token_bucket_position(256)[:64, :64].clone(), 2 * 256 - 1)}
    tables = {m: (0.5 * torch.randn(int(buckets[m].max()) + 1, heads, generator=g)).to(torch.bfloat16).float() for m in shapes}
    xs = {m: torch.randn(b, s, H, generator=g).to(torch.bfloat16).float() for m, (b, s) in shapes.items()}
    dys = {m: torch.randn(b, s, H, generator=g).to(torch.bfloat16).float() for m, (b, s) in shapes.items()}
    live = {m: (~pads[m]) if m in pads else torch.ones(b, s, dtype=torch.bool) for m, (b, s) in shapes.items()}

    def run(dev, dtype):
        sd = {"L." + k: v.detach().to(dev, dtype).clone().requires_grad_(True) for k, v in layer.state_dict().items()}
        out, dx, dt = {}, {}, {}
        for m, (b, s) in shapes.items():
            xo = xs[m].to(dev, dtype).clone().requires_grad_(True)
            tabo = tables[m].to(dev, dtype).clone().requires_grad_(True)
            bias = O.rel_pos_bias(tabo, buckets[m].to(dev)).unsqueeze(0).expand(b, -1, -1, -1)
            if m in pads:
                bias = bias.masked_fill(pads[m].to(dev)[:, None, None, :], float("-inf"))
            yo = O.encoder_layer(xo.transpose(0, 1), sd, "L", heads, m, bias).transpose(0, 1)
            (yo.float() * (dys[m] * live[m].unsqueeze(-1).float()).to(dev)).sum().backward()
            out[m], dx[m], dt[m] = yo.detach().float().cpu(), xo.grad.float().cpu(), tabo.grad.float().cpu()
        return out, dx, dt, {k[2:]: v.grad.float().cpu() for k, v in sd.items() if v.grad is not None}
    case = dict(layer=layer, shapes=shapes, pads=pads, live=live, buckets=buckets, tables=tables, xs=xs, dys=dys, H=H,
                ref=run("cpu", torch.float32), yard=run(DEV, torch.bfloat16))
    _CFG4_ORACLE[kind] = case
    return case


@pytest.mark.parametrize("route", ["bf16", "fp8", "fp8+dgrad"])
@pytest.mark.parametrize("kind", ["vl", "image1025"])
def test_config4_lengths_4b_layer_against_the_fp32_oracle(kind, route):
    """One encoder layer at the 4B dimensions at config 4's sequence lengths -- the lock-step 'vl' step (3 x 64 text tokens with ragged
    key padding + 3 x 785 image tokens: the streaming attention kernels above 384 tokens, the separate dBias kernel) and a single-stream
    2 x 1025 image pass (one segment: the gemm_nt path, no grouped launch) -- on the bf16 route and both fp8 routes
    (ops.set_fp8_ffn(True, dgrad=False / True)), against the fp32 oracle run once per modality on shared leaves: per-segment outputs
    (padded rows masked) and input gradients, the bias-table gradients and EVERY parameter gradient.  The fp8 routes count their fp8
    launches per segment: up- and down-projection (again in backward under checkpoint_activations) and the two input-gradient GEMMs."""
    import copy
    from one_peace_amd import hip, ops
    from one_peace_amd.relpos import RelPosSpec
    c = _cfg4_layer_case(kind)
    H, shapes, pads, live = c["H"], c["shapes"], c["pads"], c["live"]
    mdev = copy.deepcopy(c["layer"]).to(DEV).train()
    mdev.zero_grad()
    launches = [0]
    orig_f8 = ops.hip.gemm_nt_fp8

    def counted_f8(*a, **k):
        launches[0] += 1
        return orig_f8(*a, **k)
    old, old_dgrad = ops.FP8_FFN, ops.FP8_FFN_DGRAD
    ops.set_fp8_ffn(route != "bf16", dgrad=route == "fp8+dgrad")
    ops.hip.gemm_nt_fp8 = counted_f8
    try:
        tabs = {m: c["tables"][m].to(DEV).to(torch.bfloat16).requires_grad_(True) for m in shapes}
        dy = torch.cat([(c["dys"][m] * live[m].unsqueeze(-1).float()).reshape(-1, H) for m in shapes]).to(DEV)
        if kind == "vl":
            segs, x2, row0 = [], [], 0
            for m, (b, s) in shapes.items():
                key_pad = None
                if m in pads:
                    key_pad = torch.ones(b, hip.attn_spad(s), dtype=torch.uint8, device=DEV)
                    key_pad[:, :s] = pads[m].to(torch.uint8).to(DEV)
                segs.append(ops.StreamSeg(m, b, s, row0, RelPosSpec(tabs[m], c["buckets"][m].to(DEV)).handle(), key_pad))
                x2.append(c["xs"][m].reshape(b * s, H))
                row0 += b * s
            x2d = torch.cat(x2).to(DEV).to(torch.bfloat16).requires_grad_(True)
            y2 = mdev.forward_fused_multi(x2d, segs, None, [None] * len(segs))
        else:
            (b, s), = shapes.values()
            x2d = c["xs"]["image"].reshape(b * s, H).to(DEV).to(torch.bfloat16).requires_grad_(True)
            y2 = mdev.forward_fused(x2d.view(b, s, H), RelPosSpec(tabs["image"], c["buckets"]["image"].to(DEV)).handle(), None,
                                    "image").reshape(b * s, H)
        (y2.float() * dy).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_fp8_ffn(old, dgrad=old_dgrad)
        ops.hip.gemm_nt_fp8 = orig_f8
    recompute = bool(getattr(mdev.cfg, "checkpoint_activations", False))  # backward re-runs the forward's two fp8 GEMMs
    per_seg = 0 if route == "bf16" else 2 * (1 + recompute) + 2 * (route == "fp8+dgrad")
    assert launches[0] == per_seg * len(shapes), (launches[0], per_seg, recompute)
    (r_out, r_dx, r_dt, r_g), (t_out, t_dx, t_dt, t_g) = c["ref"], c["yard"]
    bounds = CFG4_BOUNDS[route]
    report, worst, failed = [], {}, []

    def check(cls, name, got, ref, yard):
        e, et = rel_fro(got.float().cpu(), ref), rel_fro(yard, ref)
        report.append("%-62s hip %.3e  torch-bf16 %.3e  (bound %.1e)" % (name, e, et, bounds[cls]))
        worst[cls] = max(worst.get(cls, 0.0), e)
        if not e <= bounds[cls]:
            failed.append("%s: %.3e > %.1e" % (name, e, bounds[cls]))
    row0 = 0
    for m, (b, s) in shapes.items():
        rows = slice(row0, row0 + b * s)
        row0 += b * s
        lv = live[m]
        check("out", "%s %s out %s" % (kind, route, m), y2[rows].view(b, s, H)[lv.to(DEV)], r_out[m][lv], t_out[m][lv])
        check("dx", "%s %s dx %s" % (kind, route, m), x2d.grad[rows].view(b, s, H), r_dx[m], t_dx[m])
        check("dtable", "%s %s dtable %s" % (kind, route, m), tabs[m].grad, r_dt[m], t_dt[m])
    n = 0
    for name, q in mdev.named_parameters():
        if name in r_g and float(r_g[name].norm()) > 1e-7:
            assert q.grad is not None, name
            cls = "ffn" if "_ffn." in name or name in ("gamma_2", "final_layer_norm.weight", "final_layer_norm.bias") else "grad"
            check(cls, "%s %s grad %s" % (kind, route, name), q.grad, r_g[name], t_g[name])
            n += 1
    assert n == 13 + 6 * len(shapes) + 2, n  # attention branch + gamma_1/2, one FFN set per segment, final LayerNorm
    report.append("worst per class: " + "  ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    open(os.path.join(out_dir(), "cfg4_layer_4b_parity_report_%s_%s.txt" % (kind, route.replace("+", "_"))), "w").write(
        "\n".join(report) + "\n")
    assert not failed, failed


_FLAT_ORACLE = {}


def _flat_layers_case(gamma_scale):
    """Weights, inputs, masks and the fp32 oracle's results of test_lock_step_layers_4b_under_flat_parameters... (cached per layer-scale
    magnitude: the oracle does not depend on the recompute level)."""
    if gamma_scale in _FLAT_ORACLE:
        return _FLAT_ORACLE[gamma_scale]
    from one_peace_amd.relpos import add_cls_buckets, make_image_bucket_position, make_token_bucket_position
    from one_peace_amd.transformer.transformer_layer import TransformerEncoderLayer
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    H, heads, L = 1536, 24, 2
    cfg = one_peace_encoder_config(embed_dim=H, ffn_embed_dim=6144, layers=L, attention_heads=heads, drop_path_rate=0.4)
    torch.manual_seed(0)
    layers = torch.nn.ModuleList([TransformerEncoderLayer(cfg, drop_path_rate=0.4) for _ in range(L)])
    g = torch.Generator().manual_seed(5)
    for n, q in layers.named_parameters():
        if n.endswith("gamma_1") or n.endswith("gamma_2"):  # the layer scale AROUND gamma_scale, one entry exactly 0 and one tiny
            q.data.copy_(gamma_scale * (1.0 + 0.3 * torch.randn(q.shape, generator=g)))
            q.data[5], q.data[6] = 0.0, gamma_scale * 1e-3
        elif q.dim() == 1:
            q.data.add_(0.1 * torch.randn(q.shape, generator=g))
    layers = layers.to(torch.bfloat16)  # the weights the device sees, exactly
    shapes = {"text": (8, 64), "image": (64, 257), "audio": (32, 250)}  # row counts that are multiples of 64, like the headline's
    nrel_img = (2 * 16 - 1) ** 2 + 3
    buckets = {"image": make_image_bucket_position(16, nrel_img),
               "text": add_cls_buckets(make_token_bucket_position(256)[:64, :64].clone(), 2 * 256 - 1),
               "audio": add_cls_buckets(make_token_bucket_position(512)[:250, :250].clone(), 2 * 512 - 1)}
    tables = {m: (0.5 * torch.randn(int(buckets[m].max()) + 1, heads, generator=g)).to(torch.bfloat16).float() for m in shapes}
    xs = {m: torch.randn(b, s, H, generator=g).to(torch.bfloat16).float() for m, (b, s) in shapes.items()}
    dys = {m: torch.randn(b, s, H, generator=g).to(torch.bfloat16).float() for m, (b, s) in shapes.items()}
    pads = {"audio": torch.zeros(32, 250, dtype=torch.bool)}
    pads["audio"][1, 230:] = True
    pads["audio"][7, 190:] = True
    pads["audio"][20, 64:] = True
    probs = [0.2, 0.4]  # drop-path rate of the two layers (linspace(0, 0.4, 40) ends there: transformer_encoder.py:53)
    masks = {m: torch.bernoulli(torch.full((L, 2, b), 0.7), generator=g) for m, (b, s) in shapes.items()}  # host-drawn, shared with the oracle
    for m in masks:
        masks[m][:, :, 0] = 1.0
    scales = {m: [(masks[m][i, 0] / (1 - probs[i]), masks[m][i, 1] / (1 - probs[i])) for i in range(L)] for m in shapes}
    # ---- fp32 oracle: one pass per modality over the two layers, shared leaves ----
    sdo = {"L." + k: v.detach().clone().float().requires_grad_(True) for k, v in layers.state_dict().items()}
    ref_out, ref_dx, ref_dt = {}, {}, {}
    for m, (b, s) in shapes.items():
        xo, tabo = xs[m].clone().requires_grad_(True), tables[m].clone().requires_grad_(True)
        bias_o = O.rel_pos_bias(tabo, buckets[m]).unsqueeze(0).expand(b, -1, -1, -1)
        if m in pads:
            bias_o = bias_o.masked_fill(pads[m][:, None, None, :], float("-inf"))
        h = xo.transpose(0, 1)
        for i in range(L):
            h = O.encoder_layer(h, sdo, "L.%d" % i, heads, m, bias_o, path_scale=scales[m][i])
        yo = h.transpose(0, 1)
        live = (~pads[m]).unsqueeze(-1).float() if m in pads else 1.0
        (yo * dys[m] * live).sum().backward()
        ref_out[m], ref_dx[m], ref_dt[m] = yo.detach(), xo.grad, tabo.grad
    g32 = {k[2:]: v.grad for k, v in sdo.items() if v.grad is not None}
    case = dict(layers=layers, shapes=shapes, buckets=buckets, tables=tables, xs=xs, dys=dys, pads=pads, scales=scales, ref_out=ref_out,
                ref_dx=ref_dx, ref_dt=ref_dt, g32=g32, H=H, heads=heads, L=L)
    _FLAT_ORACLE[gamma_scale] = case
    return case


@pytest.mark.parametrize("gamma_scale,cheap", [(1e-6, False), (1e-6, True), (1e-1, False), (1e-1, True)])
def test_lock_step_layers_4b_under_flat_parameters_against_the_fp32_oracle(gamma_scale, cheap):
    """Round 6 (VERDICT r5 Weak #1): the gradient route bench.py TIMES, at the headline's dimensions, against the fp32 oracle.  Two
    lock-step encoder layers (H = 1536, F = 6144, 24 heads; 8 x 64 text, 64 x 257 image, 32 x 250 audio tokens with padded keys) whose
    parameters live in distributed.FlatParameters: every gradient is accumulated IN PLACE in the flat buffer by the kernel that
    produces it, all weight gradients of a layer are ONE grouped launch, the residual GEMMs write no branch output and gamma_1 / gamma_2
    take their gradient from the weight-gradient launch's row dot (ops.dgamma_from_wgrad_ok holds: asserted), stochastic depth with
    host-drawn per-sample masks (rates 0.2 / 0.4) shared with the oracle, the layer scale drawn around 1e-6 (the reference's
    layer_scale_init_value, pretrain_vl_3B.yaml) and around 1e-1 with one entry exactly 0.0 -- where round 5's rowdot / gamma form
    returned 0 instead of the reference's sum_m ps dout y (transformer_layer.py:78-88) -- and the cheap recompute level on / off.
    Compared: per-modality outputs, input gradients, the three bias-table gradients and EVERY flat-buffer gradient."""
    import copy
    from one_peace_amd import hip, ops
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.relpos import RelPosSpec
    c = _flat_layers_case(gamma_scale)
    H, L, shapes, pads = c["H"], c["L"], c["shapes"], c["pads"]
    mdev = copy.deepcopy(c["layers"]).to(DEV).train()
    flat = FlatParameters(mdev)
    flat.zero_grad()
    old_cheap = ops.set_recompute_cheap(cheap)
    try:
        segs, x2, tabs, row0 = [], [], {}, 0
        for m, (b, s) in shapes.items():
            tabs[m] = c["tables"][m].to(DEV).to(torch.bfloat16).requires_grad_(True)
            key_pad = None
            if m in pads:
                key_pad = torch.ones(b, hip.attn_spad(s), dtype=torch.uint8, device=DEV)
                key_pad[:, :s] = pads[m].to(torch.uint8).to(DEV)
            segs.append(ops.StreamSeg(m, b, s, row0, RelPosSpec(tabs[m], c["buckets"][m].to(DEV)).handle(), key_pad))
            x2.append(c["xs"][m].reshape(b * s, H))
            row0 += b * s
        assert row0 % 64 == 0
        x2d = torch.cat(x2).to(DEV).to(torch.bfloat16).requires_grad_(True)
        h = x2d
        fused_seen = []
        orig_ok = ops.dgamma_from_wgrad_ok

        def spy(*a, **k):
            r = orig_ok(*a, **k)
            fused_seen.append(r)
            return r
        ops.dgamma_from_wgrad_ok = spy
        try:
            for i, layer in enumerate(mdev):
                ps1 = torch.cat([c["scales"][m][i][0].repeat_interleave(shapes[m][1]) for m in shapes]).to(DEV)
                ps2s = [c["scales"][m][i][1].to(DEV) for m in shapes]
                h = layer.forward_fused_multi(h, segs, ps1, ps2s)
        finally:
            ops.dgamma_from_wgrad_ok = orig_ok
        assert fused_seen and all(fused_seen), "the layer-scale gradients did not take the weight-gradient route"
        dy2 = torch.cat([(c["dys"][m] * ((~pads[m]).unsqueeze(-1).float() if m in pads else 1.0)).reshape(-1, H) for m in shapes]).to(DEV)
        (h.float() * dy2).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.set_recompute_cheap(old_cheap)
    report, worst = [], {}

    def check(kind, name, got, ref, bound):
        e = rel_fro(got.float().cpu(), ref)
        report.append("%-70s hip %.3e (bound %.1e, |ref| %.3e)" % (name, e, bound, float(ref.norm())))
        worst[kind] = max(worst.get(kind, 0.0), e)
        assert e <= bound, "%s: %.3e > %.1e" % (name, e, bound)
    for sg in segs:
        m, (b, s) = sg.name, shapes[sg.name]
        rows = slice(sg.row0, sg.end)
        live = (~pads[m]) if m in pads else torch.ones(b, s, dtype=torch.bool)
        check("out", "flat lock-step 2 x 4B layers out " + m, h[rows].view(b, s, H)[live.to(DEV)], c["ref_out"][m][live], FLAT_BOUNDS["out"])
        check("dx", "flat lock-step 2 x 4B layers dx " + m, x2d.grad[rows].view(b, s, H), c["ref_dx"][m], FLAT_BOUNDS["dx"])
        check("dtable", "flat lock-step 2 x 4B layers dtable " + m, tabs[m].grad, c["ref_dt"][m], FLAT_BOUNDS["dtable"])
    n = 0
    for name, q in mdev.named_parameters():
        ref = c["g32"].get(name)
        assert ref is not None and q.grad is not None and q.grad.data_ptr() >= flat.grads.data_ptr(), name
        kind = "gamma" if "gamma" in name else "grad"
        check(kind, "flat lock-step 2 x 4B layers grad " + name, q.grad, ref, FLAT_BOUNDS[kind])
        if "gamma" in name:  # the zero and the tiny layer-scale entry, element by element: the reference's value, not 0
            for col in (5, 6):
                got, want = float(q.grad[col]), float(ref[col])
                scale = float(ref.abs().median())
                report.append("%-70s [%d] got %.4e want %.4e" % (name, col, got, want))
                assert abs(got - want) <= 4e-2 * abs(want) + 2e-2 * scale, (name, col, got, want)
        n += 1
    assert n == 2 * 33, n  # per layer: attention branch 12 (incl. gamma_1), three FFN sets 6 each, final LayerNorm 2, gamma_2
    report.append("worst per class: " + "  ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out",
                      "flat_layers_4b_parity_report_gamma%g_cheap%d.txt" % (gamma_scale, int(cheap))), "w").write("\n".join(report) + "\n")


# 2.5 x the largest error measured per class over the four cases (profiles/r6_flat_layers_4b_parity_report_*.txt: out 3.3e-3, dx 3.8e-3,
# bias tables 6.5e-3, parameter gradients 8.1e-3, layer scales 5.9e-3)
FLAT_BOUNDS = {"out": 8.2e-3, "dx": 9.5e-3, "dtable": 1.6e-2, "grad": 2.0e-2, "gamma": 1.5e-2}


# 2.5 x the largest error measured per class (profiles/r6_audio_15s_4b_parity_report_{audio,al}.txt: out 2.4e-3, dx 2.5e-3, bias tables
# 5.7e-3, parameter gradients 6.7e-3)
LONG_AUDIO_BOUNDS = {"out": 6.1e-3, "dx": 6.4e-3, "dtable": 1.4e-2, "grad": 1.7e-2}


@pytest.mark.parametrize("stream", ["audio", "al"])
def test_reference_audio_length_15s_4b_layer_against_the_fp32_oracle(stream):
    """Round 6 (VERDICT r5 Missing #2): the reference's own audio length -- pretrain_al_3B.yaml:10 max_duration 15 s = 750 tokens, the
    `al` joint stream 72 text + 750 audio = 822 tokens (transformer_encoder.py:144-162, transformer_layer.py:214-217) -- through one
    encoder layer at the 4B dimensions with RAGGED key padding, forward and backward, against the fp32 oracle.  These lengths leave
    the persistent attention kernels (193 ... 257 tokens) for the streaming ones; the joint stream reads the block-diagonal bias (text
    table | audio table, zero across) and routes each row range through its own FFN."""
    from one_peace_amd import hip
    from one_peace_amd.relpos import RelPosSpec, add_cls_buckets, joint_handle, make_token_bucket_position
    from one_peace_amd.transformer.transformer_layer import TransformerEncoderLayer
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    H, heads = 1536, 24
    cfg = one_peace_encoder_config(embed_dim=H, ffn_embed_dim=6144, layers=1, attention_heads=heads, drop_path_rate=0.0)
    torch.manual_seed(0)
    layer = TransformerEncoderLayer(cfg, drop_path_rate=0.0)
    g = torch.Generator().manual_seed(9)
    for n, q in layer.named_parameters():
        if q.dim() == 1:
            q.data.add_(0.1 * torch.randn(q.shape, generator=g))
    layer = layer.to(torch.bfloat16)
    Sa, St = 750, 72
    bk_a = add_cls_buckets(make_token_bucket_position(512)[:Sa, :Sa].clone(), 2 * 512 - 1)
    bk_t = add_cls_buckets(make_token_bucket_position(256)[:St, :St].clone(), 2 * 256 - 1)
    tab_a = (0.5 * torch.randn(int(bk_a.max()) + 1, heads, generator=g)).to(torch.bfloat16).float()
    tab_t = (0.5 * torch.randn(int(bk_t.max()) + 1, heads, generator=g)).to(torch.bfloat16).float()
    if stream == "audio":
        B, S = 4, Sa
        lens = [750, 701, 333, 64]            # frames of each clip incl. CLS: the rest is padding
        pad = torch.arange(S)[None, :] >= torch.tensor(lens)[:, None]
    else:
        B, S = 3, St + Sa
        tl, al = [72, 40, 13], [750, 518, 97]  # text tokens / audio frames of each pair; padding sits at the end of EACH segment
        pad = torch.cat([torch.arange(St)[None, :] >= torch.tensor(tl)[:, None], torch.arange(Sa)[None, :] >= torch.tensor(al)[:, None]], 1)
    x = torch.randn(B, S, H, generator=g).to(torch.bfloat16).float()
    dy = torch.randn(B, S, H, generator=g).to(torch.bfloat16).float() * (~pad).unsqueeze(-1).float()
    # ---- fp32 oracle ----
    sdo = {"L." + k: v.detach().clone().float().requires_grad_(True) for k, v in layer.state_dict().items()}
    xo, ta, tt = x.clone().requires_grad_(True), tab_a.clone().requires_grad_(True), tab_t.clone().requires_grad_(True)
    if stream == "audio":
        bias_o = O.rel_pos_bias(ta, bk_a).unsqueeze(0).expand(B, -1, -1, -1)
        kw = {}
    else:
        blk = torch.zeros(heads, S, S)
        bias_o = (torch.nn.functional.pad(O.rel_pos_bias(tt, bk_t), (0, Sa, 0, Sa)) + torch.nn.functional.pad(O.rel_pos_bias(ta, bk_a), (St, 0, St, 0))
                  + blk).unsqueeze(0).expand(B, -1, -1, -1)
        kw = dict(text_seq_len=St, audio_seq_len=Sa)
    bias_o = bias_o.masked_fill(pad[:, None, None, :], float("-inf"))
    yo = O.encoder_layer(xo.transpose(0, 1), sdo, "L", heads, stream, bias_o, **kw).transpose(0, 1)
    (yo * dy).sum().backward()
    g32 = {k[2:]: v.grad for k, v in sdo.items() if v.grad is not None}
    # ---- HIP ----
    m = layer.to(DEV)
    m.zero_grad()
    xd = x.to(DEV).to(torch.bfloat16).requires_grad_(True)
    tad, ttd = tab_a.to(DEV).to(torch.bfloat16).requires_grad_(True), tab_t.to(DEV).to(torch.bfloat16).requires_grad_(True)
    key_pad = torch.ones(B, hip.attn_spad(S), dtype=torch.uint8, device=DEV)
    key_pad[:, :S] = pad.to(torch.uint8).to(DEV)
    if stream == "audio":
        y = m.forward_fused(xd, RelPosSpec(tad, bk_a.to(DEV)).handle(), key_pad, "audio")
    else:
        handle = joint_handle([RelPosSpec(ttd, bk_t.to(DEV)), RelPosSpec(tad, bk_a.to(DEV))], [St, Sa])
        y = m.forward_fused(xd, handle, key_pad, "al", seg_lens=(St, Sa))
    (y.float() * dy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    report, worst = [], {}

    def check(kind, name, got, ref):
        e = rel_fro(got.float().cpu(), ref)
        bound = LONG_AUDIO_BOUNDS[kind]
        report.append("%-70s hip %.3e (bound %.1e)" % (name, e, bound))
        worst[kind] = max(worst.get(kind, 0.0), e)
        assert e <= bound, "%s: %.3e > %.1e" % (name, e, bound)
    live = ~pad
    check("out", "%s 15 s 4B layer out" % stream, y[live.to(DEV)], yo.detach()[live])
    check("dx", "%s 15 s 4B layer dx" % stream, xd.grad[live.to(DEV)], xo.grad[live])
    check("dtable", "%s 15 s 4B layer dtable audio" % stream, tad.grad, ta.grad)
    if stream == "al":
        check("dtable", "al 15 s 4B layer dtable text", ttd.grad, tt.grad)
    n = 0
    for name, q in m.named_parameters():
        ref = g32.get(name)
        if ref is not None and float(ref.norm()) > 1e-7:
            assert q.grad is not None, name
            check("grad", "%s 15 s 4B layer grad %s" % (stream, name), q.grad, ref)
            n += 1
    assert n >= (26 if stream == "al" else 20), n
    report.append("worst per class: " + "  ".join("%s %.3e" % kv for kv in sorted(worst.items())))
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "audio_15s_4b_parity_report_%s.txt" % stream), "w").write(
        "\n".join(report) + "\n")


def test_sample_prefetcher_matches_prepare_sample():
    """staging.SamplePrefetcher == trainer.py:1297-1336 (_prepare_sample: move_to_cuda + fp32->bf16 of floating tensors,
    integer / bool tensors untouched, nested dict structure kept), for a stream of different samples and slot reuse."""
    from one_peace_amd.staging import SamplePrefetcher
    g = torch.Generator().manual_seed(0)

    def make(i):
        return {"id": torch.tensor([i]), "nsentences": 4,
                "net_input": {"src_tokens": torch.randint(0, 1000, (4, 9), generator=g),
                              "src_images": torch.randn(4, 3, 32, 32, generator=g) + i,
                              "audio_padding_masks": torch.zeros(4, 7, dtype=torch.bool)}}
    samples = [make(i) for i in range(5)]
    got = list(SamplePrefetcher(iter(samples), DEV))
    assert len(got) == 5
    for s_host, s_dev in zip(samples, got):
        assert s_dev["nsentences"] == 4 and int(s_dev["id"].item()) == int(s_host["id"].item())
        ni, nd = s_host["net_input"], s_dev["net_input"]
        assert nd["src_tokens"].dtype == torch.int64 and torch.equal(nd["src_tokens"].cpu(), ni["src_tokens"])
        assert nd["audio_padding_masks"].dtype == torch.bool
        assert nd["src_images"].dtype == torch.bfloat16 and nd["src_images"].is_cuda
        assert torch.equal(nd["src_images"].cpu(), ni["src_images"].to(torch.bfloat16))


@pytest.mark.parametrize("stage", ["vl", "al"])
def test_full_pretraining_objective_on_hip(golden_dir, stage):
    """The complete image-text pretraining step (ITC + four DCL terms; six encoder passes, three of them with per-sample
    preserve ids, three decoder passes; image_text_pretrain_loss.py:76-160) on the HIP path: every encoder / decoder pass
    must take the fused layers (per-sample bias images for the masked passes), the DCL similarity is computed blockwise,
    and losses / gradients are held to the reference-written fixture with the usual bf16 yardstick."""
    from tests.test_model_cpu import _build_pretrain
    from one_peace_amd.criterions.pretrain import AudioTextPretrainLossCriterion, ImageTextPretrainLossCriterion
    from one_peace_amd.transformer import transformer_encoder as TE
    fx = _fx(golden_dir, "micro_pretrain.pt" if stage == "vl" else "micro_pretrain_al.pt")
    ni = {k: (v.to(DEV).to(torch.bfloat16) if v.is_floating_point() else v.to(DEV)) for k, v in fx["net_input"].items()}
    calls = {"fused": 0, "torch": 0}
    from one_peace_amd import ops as _ops
    dense_inits = []
    orig_dense_init = _ops.DenseBias.__init__

    def _no_dense(self, dense):  # the masked passes must build their per-sample images from position ids, never from a dense
        dense_inits.append(tuple(dense.shape))  # [B, heads, K, K] tensor (adapter/image.py:188-204 is replaced, not ported)
        orig_dense_init(self, dense)
    _ops.DenseBias.__init__ = _no_dense
    of, ot, om = TE.TransformerEncoder._forward_fused, TE.TransformerEncoder._forward_torch, TE.TransformerEncoder.forward_multi

    def cf(self, *a, **k):
        calls["fused"] += 1
        return of(self, *a, **k)

    def cm(self, infos):
        calls["multi"] = calls.get("multi", 0) + len(infos)
        return om(self, infos)

    def ct(self, *a, **k):
        calls["torch"] += 1
        return ot(self, *a, **k)

    res = {}
    TE.TransformerEncoder._forward_fused, TE.TransformerEncoder._forward_torch, TE.TransformerEncoder.forward_multi = cf, ct, cm
    try:
        for mode in ("hip", "torch"):
            m = _build_pretrain(fx, audio_language=stage == "al").to(DEV).to(torch.bfloat16).eval()
            _force_torch_path(m, mode == "torch")
            calls["fused"] = calls["torch"] = calls["multi"] = 0
            crit = (ImageTextPretrainLossCriterion(None, 0.5, 1.0, 0.5, 0.5, 2.5, label_smoothing=0.0) if stage == "vl"
                    else AudioTextPretrainLossCriterion(None, 1.0, 0.5, 0.5, 2.5, label_smoothing=0.0))
            loss, _, log = crit(m, {"net_input": ni, "nsentences": 4})
            m.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
            if mode == "hip":
                # vl: 6 encoder + 3 decoder passes; al: 5 encoder + 2 decoder passes -- all on the fused layers (round 4: the two unmasked
                # single-modality passes of the vl objective as ONE lock-step pass)
                assert calls["torch"] == 0 and calls["fused"] + calls["multi"] == (9 if stage == "vl" else 7), calls
                assert calls["multi"] == (2 if stage == "vl" else 0), calls
            res[mode] = dict(log={k: float(v) for k, v in log.items() if "loss" in k},
                             grads={n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None})
    finally:
        TE.TransformerEncoder._forward_fused, TE.TransformerEncoder._forward_torch, TE.TransformerEncoder.forward_multi = of, ot, om
        _ops.DenseBias.__init__ = orig_dense_init
    assert not dense_inits, "dense per-sample bias tensors were built: %s" % dense_inits
    report = []
    for k, ref in fx["log"].items():
        if "loss" in k:
            eh, et = abs(res["hip"]["log"][k] - float(ref)), abs(res["torch"]["log"][k] - float(ref))
            report.append("%-20s ref %.5f hip err %.2e torch-bf16 err %.2e" % (k, float(ref), eh, et))
            assert eh <= 3e-2 * max(1.0, abs(float(ref))), (k, eh, et)  # absolute
    n_checked = 0
    for k, v in fx["grads"].items():
        if k.endswith("#norm") or k.endswith("#rows4"):
            continue
        if float(v.norm()) < 1e-7 or k not in res["hip"]["grads"]:
            continue
        gh, gt = res["hip"]["grads"][k], res["torch"]["grads"][k]
        if v.dim() == 1 and float(v.norm()) < 0.1:
            # bias-type gradients of the 64-wide decoder are sums of strongly cancelling rows (v_proj.bias is exactly
            # sum_q dO_q because softmax rows sum to one; norm ~5e-2 against summands ~1): their RELATIVE error is
            # meaningless -- hold the absolute error to 2e-2, below what 6e-2 relative allows on the typical
            # (norm 0.5) gradient of this model (measured 1.2e-2 / 4e-3).  The attention kernels themselves reproduce colsum(dV) to 9e-4.
            e_abs = float((gh - v).norm())
            report.append("%-60s |hip - ref| %.3e (|ref| %.3e)" % ("grad " + k, e_abs, float(v.norm())))
            assert e_abs <= 2e-2, (k, e_abs)
        else:
            _check("grad " + k, gh, gt, v, 6e-2, report)
        n_checked += 1
    assert n_checked > 40
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "pretrain_%s_parity_report.txt" % stage), "w").write(
        "\n".join(report) + "\n")


def test_fused_adamw_with_layer_decay_groups_matches_reference_optimizer(golden_dir):
    """tests/golden/optim.pt = the reference's Adam + clip_grad_norm_ + layer-decay param groups run for three steps on the bf16
    micro model (generated through ref_shim).  FusedAdamW over FlatParameters with the same groups (one launch per step, per-range
    lr table) must land on the same parameters: every norm within 2e-4 relative, every stored element within one bf16 ulp (+ 1.5e-5 absolute)
    (the reference rounds the clipped gradient to bf16 before Adam; the fused kernel applies the clip coefficient in fp32)."""
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import FusedAdamW, reference_param_groups
    fx = _fx(golden_dir, "optim.pt")
    cfg, oc = fx["cfg"], fx["optim"]
    m = load_synth(build_retrieval(dict(cfg), fx["vocab"]), fx["shapes"]).to(DEV).to(torch.bfloat16)
    no_decay, lr_scale = reference_param_groups(m, cfg["layers"], oc["layer_decay"])
    flat = FlatParameters(m, no_decay=no_decay, lr_scale=lr_scale)
    by_name = {n: (o, k) for n, _, o, k in flat.entries}
    for start, end, scale, decays in flat.groups:  # the reference's group of every parameter (lr_scale, weight decay)
        for n, (o, k) in by_name.items():
            if start <= o < end:
                want_scale, want_wd = fx["assign"][n]
                assert abs(scale - want_scale) < 1e-12 and (oc["weight_decay"] if decays else 0.0) == want_wd, n
    assert len([g for g in flat.groups if g[1] > g[0]]) == len(set(fx["assign"].values()))
    opt = FusedAdamW(flat, lr=oc["lr"][0], betas=oc["betas"], eps=oc["eps"], weight_decay=oc["weight_decay"])
    for step, lr in enumerate(oc["lr"], start=1):
        opt.zero_grad()
        for n, p in m.named_parameters():
            p.grad.copy_(synth.optim_grad(n, p.shape, step).to(DEV))
        opt.set_lr(lr)
        norm = opt.step(clip_norm=oc["clip_norm"])
        torch.cuda.synchronize()
        assert abs(float(norm) - float(fx["grad_norms"][step - 1])) <= 1e-3 * float(fx["grad_norms"][step - 1])
        snap = fx["params_after"][step - 1]
        for n, p in m.named_parameters():
            got = p.detach().float().cpu()
            want_norm = float(snap[n + "#norm"])
            assert abs(float(got.double().norm()) - want_norm) <= 2e-4 * want_norm + 1e-6, (step, n)
            ref = (snap[n] if n in snap else snap[n + "#head"]).float().reshape(-1)
            g = got.reshape(-1)[: ref.numel()]
            # one bf16 ulp of the parameter, plus 0.5 % of the largest possible update (lr * sqrt(1-b2)/(1-b1) ~ 3e-3): where the
            # update nearly cancels the parameter, the 2^-9 relative difference of the clipped gradient is all that is left
            # (one ulp PER STEP: a parameter that rounded the other way keeps that offset in the following steps)
            tol = step * torch.maximum(ref.abs(), g.abs()) * 2.0 ** -7 + 1.5e-5
            assert ((g - ref).abs() <= tol).all(), (step, n, float(((g - ref).abs() / tol).max()))


def test_batched_weight_cache_refresh_after_optimizer_step():
    """optim.FusedAdamW updates the flat parameters through raw pointers and then rebuilds every cached transposed weight
    (the dgrad operands, incl. the fused q|k|v one) in ONE batched launch: after each step every cache entry must equal
    the transpose of the just-updated weights, and training must follow the lazily-refreshed path exactly."""
    from one_peace_amd import ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import FusedAdamW
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=2, attention_heads=2, image_rel_bucket_size=4,
               text_bucket_size=256, audio_bucket_size=512)
    inp = _to_dev(synth.synth_inputs(8, text_len=15, image_res=64, audio_samples=8000, vocab=1000))
    losses = {}
    for mode in ("batched", "lazy"):
        m = load_synth(build_retrieval(cfg, 1000)).to(DEV).to(torch.bfloat16).eval()
        flat = FlatParameters(m)
        opt = FusedAdamW(flat, lr=1e-3)
        orig = ops.refresh_weight_cache
        if mode == "lazy":
            ops.refresh_weight_cache = ops.invalidate_weight_cache
        try:
            out = []
            for _ in range(3):
                opt.zero_grad()
                loss, _, _ = TriModalContrastiveCriterion(None, 0.0)(m, {"net_input": inp, "nsentences": 8})
                loss.backward()
                opt.step(clip_norm=3.0)
                out.append(float(loss.detach()))
                if mode == "batched":
                    n = 0
                    for key, (refs, ver, t, sref) in ops._wt_cache.items():
                        ws = [r() for r in refs]
                        if any(w is None for w in ws) or not any(w is p for w in ws for p in m.parameters()):
                            continue
                        assert ver[2] == ops._cache_epoch
                        want = torch.cat([w.detach() for w in ws], 0)
                        if sref is not None:  # the last Linear of a residual branch: the layer scale is folded into the copy
                            want = (want.float() * sref().detach().float()[:, None]).to(torch.bfloat16)
                        assert torch.equal(t, want.t()), key
                        n += 1
                    assert n >= 2 * 6  # per layer: q|k|v, out, 3 x (wi_0, wi_1, w2) of the modality actually used ...
        finally:
            ops.refresh_weight_cache = orig
        losses[mode] = out
    assert losses["batched"] == losses["lazy"], losses


@pytest.mark.parametrize("fp8", [False, True])
def test_weight_copies_follow_torch_updates_of_ordinary_parameters(fp8):
    """The derived weight copies (transposed bf16 dgrad operands and, with fp8 and its input-gradient GEMMs on, their e4m3 copies) after
    updates that do NOT go through FusedAdamW: a torch.optim.SGD step, load_state_dict from another state and an in-place edit of every
    gamma_2 (folded into the transposed down-projection copy).  After each, the step's loss and every gradient must be bit for bit those
    of the same step on the same weights with every cache emptied.  fp8=False is the control."""
    from one_peace_amd import ops as _ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=256, ffn_embed_dim=512, layers=2, attention_heads=4, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B = 5
    inp = _to_dev(synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000))

    def model(seed):
        enc = one_peace_encoder_config(drop_path_rate=0.0, layer_scale_init_value=1e-1, checkpoint_activations=False, **cfg)
        torch.manual_seed(seed)
        m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
        return m.to(DEV).to(torch.bfloat16).train()
    m = model(0)
    other = model(1)
    with torch.no_grad():
        for q in other.parameters():
            q.add_(0.05 * torch.randn_like(q))  # load_synth gives the same synthetic weights: make the other state differ
    other_state = {k: v.clone() for k, v in other.state_dict().items()}
    del other
    crit = TriModalContrastiveCriterion(None, 0.0)
    launches = [0]
    orig_f8 = _ops.hip.gemm_nt_fp8

    def counted_f8(*a, **k):
        launches[0] += 1
        return orig_f8(*a, **k)

    def step():
        m.zero_grad()
        loss, _, _ = crit(m, {"net_input": inp, "nsentences": B})
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach().clone(), {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None}

    def empty_caches():
        for c in (_ops._wt_cache, _ops._fp8_cache, _ops._fp8_pairs, _ops._fp8_derived_cache):
            c.clear()
        _ops._refresh_plan = None

    def sgd():
        w2 = next(q for n, q in m.named_parameters() if n.endswith("image_ffn.3.weight"))
        before = w2.detach().clone()
        torch.optim.SGD(m.parameters(), lr=0.3).step()  # on the gradients of the last step
        assert not torch.equal(before, w2.detach()), "the SGD step left the weights unchanged"

    def gamma_2():
        with torch.no_grad():
            for n, q in m.named_parameters():
                if n.endswith("gamma_2"):
                    q.mul_(1.5)
    old, old_dgrad = _ops.FP8_FFN, _ops.FP8_FFN_DGRAD
    _ops.set_fp8_ffn(fp8, dgrad=True)
    _ops.hip.gemm_nt_fp8 = counted_f8
    try:
        empty_caches()
        step()
        for what, update in (("SGD step", sgd), ("load_state_dict", lambda: m.load_state_dict(other_state)), ("gamma_2 edit", gamma_2)):
            update()
            launches[0] = 0
            loss, grads = step()
            assert launches[0] == (2 * 3 * 4 if fp8 else 0), launches[0]  # 2 layers x 3 modalities x (up, down, dy W2, dh W01)
            empty_caches()
            loss_f, grads_f = step()
            assert torch.equal(loss, loss_f), (what, float(loss), float(loss_f))
            assert grads.keys() == grads_f.keys()
            bad = [n for n in grads if not torch.equal(grads[n], grads_f[n])]
            assert not bad, (what, bad)
    finally:
        _ops.set_fp8_ffn(old, dgrad=old_dgrad)
        _ops.hip.gemm_nt_fp8 = orig_f8


def test_masked_image_pass_with_more_than_384_kept_tokens_takes_the_fused_path():
    """Masked image pass of the pretraining objective at 448^2 (785 tokens) keeping CLS + 499 patches per sample -- a different
    subset per sample, so the relative-position bias is one image per sample and its gradient one slab per sample
    (adapter/image.py:188-204,229-246).  Up to round 2 more than 384 kept tokens fell back to the torch layers (the per-sample
    bias gradient existed only in the merged dQ + dBias kernel); now the separate dQ / dBias kernels write per-sample slabs.
    Checked: the fused layers run (no torch fallback), and features + every gradient (incl. the relative-position table's)
    against the mirror's reference-algorithm path in fp32 on the same weights; the masked passes' parity with the reference
    itself is pinned at small sizes by the golden pretraining fixtures."""
    from one_peace_amd.transformer import transformer_encoder as TE
    grid, keep = 28, 500
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=2, attention_heads=2, image_bucket_size=grid,
               image_rel_bucket_size=grid, text_bucket_size=256, audio_bucket_size=512)
    g = torch.Generator().manual_seed(5)
    imgs = torch.randn(3, 3, 448, 448, generator=g)
    # preserve ids index the token sequence WITH its CLS token at 0, which is always kept (data side of the reference)
    ids = torch.stack([torch.cat([torch.zeros(1, dtype=torch.long), 1 + torch.randperm(grid * grid, generator=g)[:keep - 1].sort().values])
                       for _ in range(3)])
    w = torch.randn(3, keep, 128, generator=g)
    calls = {"fused": 0, "torch": 0}
    of, ot = TE.TransformerEncoder._forward_fused, TE.TransformerEncoder._forward_torch

    def cf(self, *a, **k):
        calls["fused"] += 1
        return of(self, *a, **k)

    def ct(self, *a, **k):
        calls["torch"] += 1
        return ot(self, *a, **k)

    res = {}
    TE.TransformerEncoder._forward_fused, TE.TransformerEncoder._forward_torch = cf, ct
    try:
        for mode, dt in (("hip", torch.bfloat16), ("torch", torch.bfloat16), ("fp32", torch.float32)):
            m = load_synth(build_retrieval(cfg, 1000)).to(DEV).to(dt).eval()
            _force_torch_path(m, mode != "hip")
            calls["fused"] = calls["torch"] = 0
            feats = m.encoder_wrapper(src_images=imgs.to(DEV).to(dt), image_preserve_ids=ids.to(DEV), encoder_type="image")[1]
            assert feats.shape == (3, keep, 128)
            if mode == "hip":
                assert calls == {"fused": 1, "torch": 0}, calls
            m.zero_grad()
            (feats.float() * w.to(DEV)).sum().backward()
            res[mode] = (feats.detach().float().cpu(),
                         {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None})
    finally:
        TE.TransformerEncoder._forward_fused, TE.TransformerEncoder._forward_torch = of, ot
    report = []
    _check("masked 448^2 image features (500 kept tokens)", res["hip"][0], res["torch"][0], res["fp32"][0], 1.5e-2, report)
    n = 0
    for k, ref in res["fp32"][1].items():
        if k in res["hip"][1] and float(ref.norm()) > 1e-7:
            _check("grad " + k, res["hip"][1][k], res["torch"][1][k], ref, 5e-2, report, abs_err=1.5e-3)
            n += 1
    assert n > 30 and any("rel_pos_table" in k for k in res["hip"][1])
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "masked_448_parity_report.txt"), "w").write("\n".join(report) + "\n")


@pytest.mark.parametrize("res_px", [448, 512])
def test_long_sequence_image_on_hip(res_px):
    """BASELINE configs[4] shape class: 448^2 images -> 28 x 28 patches + CLS = 785 tokens and 512^2 -> 1025 tokens (the
    streaming attention kernels with 13 / 17 key tiles, separate dQ / dBias kernels, 2-D relative-position buckets at the
    larger grid), image tower forward + backward of a small-width model, HIP against the fp32 CPU oracle."""
    grid = res_px // 16
    S = grid * grid + 1
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=2, attention_heads=2, image_bucket_size=grid,
               image_rel_bucket_size=grid, text_bucket_size=256, audio_bucket_size=512)
    g = torch.Generator().manual_seed(3)
    imgs = torch.randn(2, 3, res_px, res_px, generator=g)
    res = {}
    w = torch.randn(2, S, 128, generator=torch.Generator().manual_seed(4))
    for mode in ("hip", "torch"):
        m = load_synth(build_retrieval(cfg, 1000)).to(DEV).to(torch.bfloat16).eval()
        _force_torch_path(m, mode != "hip")
        feats = m.encoder_wrapper(src_images=imgs.to(DEV).to(torch.bfloat16), encoder_type="image")[1]
        assert feats.shape == (2, S, 128)
        m.zero_grad()
        (feats.float() * w.to(DEV)).sum().backward()
        res[mode] = (feats.detach().float().cpu(),
                     {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None})
    # fp32 reference: the CPU oracle on the same synthetic weights (buffers -- bucket tables, position ids -- from the mirror)
    m32 = load_synth(build_retrieval(cfg, 1000))
    sd = {k: (v.detach().clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in m32.state_dict().items()}
    fo = O.model_wrapper_forward(sd, "encoder_wrapper", cfg["attention_heads"], cfg["layers"], "image", src_images=imgs)[0]["image"]
    (fo * w).sum().backward()
    res["fp32"] = (fo.detach(), {k: v.grad for k, v in sd.items() if torch.is_tensor(v) and v.requires_grad and v.grad is not None})
    report = []
    _check("%d^2 image features" % res_px, res["hip"][0], res["torch"][0], res["fp32"][0], 1.5e-2, report)
    n = 0
    for k, ref in res["fp32"][1].items():
        if k in res["hip"][1] and float(ref.norm()) > 1e-7:
            _check("grad " + k, res["hip"][1][k], res["torch"][1][k], ref, 5e-2, report, abs_err=1.5e-3)
            n += 1
    assert n > 30 and any("rel_pos_table" in k for k in res["hip"][1])


def test_deep_vision_branch_8_layers_4b_dimensions(golden_dir):
    """tests/golden/deep_vision.pt: the reference's image-only retrieval model at the 4B layer dimensions (H=1536, F=6144, 24
    heads), EIGHT layers deep, two 256^2 images, run on CPU in fp32 through ref_shim.  The HIP path in bf16 must reproduce the
    normalised CLS embeddings, the first feature rows and every parameter-gradient norm of loss = sum(logits * w).
    Stated, ABSOLUTE tolerances (bf16 storage, 8 layers; one 4B-dimension layer measures 3e-3, test_full_size_layer_4b_dimensions):
    embeddings rel-Frobenius <= 2e-2 and cosine >= 0.9998 per sample; features <= 2e-2; gradient norms within 2 %, small
    gradients (<= 1536 elements) rel-Frobenius <= 5e-2 + 1.5e-3 absolute.  Measured on MI355X: 1.31e-2 / 0.99991 / 1.30e-2 / 0.4 % /
    1.6e-2 (profiles/r2_deep_vision_parity_report.txt).  The bf16 torch path of the mirror is reported next to it (not a gate)."""
    fx = _fx(golden_dir, "deep_vision.pt")
    imgs = synth.synth_inputs(fx["batch"], image_res=fx["image_res"], vocab=fx["vocab"])["src_images"]
    w = synth.synth_tensor("deep/w", fx["logits"].shape, seed=5)
    out = {}
    for mode in ("hip", "torch"):
        m = load_synth(build_retrieval(dict(fx["cfg"]), fx["vocab"], head_type="image"), fx["shapes"]).to(DEV).to(torch.bfloat16).eval()
        _force_torch_path(m, mode == "torch")
        x = imgs.to(DEV).to(torch.bfloat16)
        logits = m(src_images=x, encoder_type="image")
        feats = m.encoder_wrapper(src_images=x, encoder_type="image")[1]
        m.zero_grad()
        (logits.float() * w.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        out[mode] = (logits.detach().float().cpu(), feats[:, :4].detach().float().cpu(),
                     {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None})
        del m
        torch.cuda.empty_cache()
    report = []
    for mode in ("hip", "torch"):
        lg, ft, gr = out[mode]
        e_l, e_f = rel_fro(lg, fx["logits"]), rel_fro(ft, fx["feats_head"])
        cos = torch.nn.functional.cosine_similarity(lg, fx["logits"], dim=1).min()
        worst_n, worst_s = 0.0, 0.0
        for k, ref in fx["grads"].items():
            if k.endswith("#norm"):
                n = k[:-5]
                if float(ref) > 1e-6:
                    worst_n = max(worst_n, abs(float(gr[n].double().norm()) - float(ref)) / float(ref))
            elif float(ref.norm()) > 1e-6:
                worst_s = max(worst_s, (float((gr[k] - ref).double().norm()) - 1.5e-3) / float(ref.double().norm()))
        report.append("%-6s logits rel-fro %.3e cos %.6f | feats %.3e | worst grad-norm dev %.3e | worst small-grad rel-fro (after abs slack) %.3e"
                      % (mode, e_l, float(cos), e_f, worst_n, worst_s))
        if mode == "hip":
            assert e_l <= 2e-2 and float(cos) >= 0.9998, report[-1]
            assert e_f <= 2e-2, report[-1]
            assert worst_n <= 2e-2 and worst_s <= 5e-2, report[-1]
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "deep_vision_parity_report.txt"), "w").write(
        "\n".join(report) + "\n")


def test_deep_text_and_audio_towers_8_layers_4b_dimensions_with_backward(golden_dir):
    """tests/golden/deep_text_audio.pt (round 4): the reference's text and audio towers at the 4B layer dimensions, EIGHT layers
    deep, three captions (padded rows) and three two-second clips, WITH the backward of loss = sum(text_logits * w_t) +
    sum(audio_logits * w_a).  The HIP path in bf16 must reproduce both normalised embeddings, the first feature rows, every
    parameter-gradient norm, the small gradients and the row probes of the large ones.  Same absolute tolerances as the 8-layer
    image fixture: embeddings rel-Frobenius <= 2e-2 and cosine >= 0.9998, features <= 2e-2, gradient norms within 2 % (3 % below a
    norm of 1e-3), element-wise probes rel-Frobenius <= 5e-2 + 1.5e-3 absolute (no exemptions)."""
    fx = _fx(golden_dir, "deep_text_audio.pt")
    inp = _to_dev(synth.synth_inputs(fx["batch"], text_len=fx["text_len"], audio_samples=fx["audio_samples"], vocab=fx["vocab"]))
    wt = synth.synth_tensor("deep_ta/wt", fx["text_logits"].shape, seed=6).to(DEV)
    wa = synth.synth_tensor("deep_ta/wa", fx["audio_logits"].shape, seed=7).to(DEV)
    out = {}
    from one_peace_amd.distributed import FlatParameters
    for mode in ("hip", "hip-flat", "torch"):  # hip-flat (round 6): the gradients accumulate in place in distributed.FlatParameters, the
        m = load_synth(build_retrieval(dict(fx["cfg"]), fx["vocab"], head_type="al"), fx["shapes"]).to(DEV).to(torch.bfloat16).eval()
        _force_torch_path(m, mode == "torch")  # route bench.py times -- here with the audio adapter (first conv block fused from the waveform)
        flat = FlatParameters(m) if mode == "hip-flat" else None
        t = m(src_tokens=inp["src_tokens"], encoder_type="text")
        a = m(src_audios=inp["src_audios"], audio_padding_masks=inp["audio_padding_masks"], encoder_type="audio")
        with torch.no_grad():
            ft = m.encoder_wrapper(src_tokens=inp["src_tokens"], encoder_type="text")[0]
            fa = m.encoder_wrapper(src_audios=inp["src_audios"], audio_padding_masks=inp["audio_padding_masks"], encoder_type="audio")[2]
        (flat or m).zero_grad()
        ((t.float() * wt).sum() + (a.float() * wa).sum()).backward()
        torch.cuda.synchronize()
        out[mode] = (t.detach().float().cpu(), a.detach().float().cpu(), ft[:, :4].float().cpu(), fa[:, :4].float().cpu(),
                     {n: p.grad.detach().float().cpu() for n, p in m.named_parameters() if p.grad is not None})
        del m, flat
        torch.cuda.empty_cache()
    report = []
    for mode in ("hip", "hip-flat", "torch"):
        t, a, ft, fa, gr = out[mode]
        e_t, e_a = rel_fro(t, fx["text_logits"]), rel_fro(a, fx["audio_logits"])
        cos = min(float(torch.nn.functional.cosine_similarity(t, fx["text_logits"], dim=1).min()),
                  float(torch.nn.functional.cosine_similarity(a, fx["audio_logits"], dim=1).min()))
        e_f = max(rel_fro(ft, fx["text_feats_head"]), rel_fro(fa, fx["audio_feats_head"]))
        worst_n, worst_s, worst_name = 0.0, 0.0, ""
        for k, ref in fx["grads"].items():
            if k.endswith("#norm"):
                n = k[:-5]
                r = float(ref)
                if r > 1e-6:
                    dev = abs(float(gr[n].double().norm()) - r) / r / (1.5 if r < 1e-3 else 1.0)
                    worst_n = max(worst_n, dev)
            else:
                n = k[:-6] if k.endswith("#rows4") else k
                got = gr[n][:4] if k.endswith("#rows4") else gr[n]
                if float(ref.norm()) > 1e-6:
                    e = (float((got - ref).double().norm()) - 1.5e-3) / float(ref.double().norm())
                    if e > worst_s:
                        worst_s, worst_name = e, k
        report.append("%-8s logits rel-fro %.3e / %.3e cos %.6f | feats %.3e | worst grad-norm dev %.3e | worst probe rel-fro (after abs slack) %.3e %s"
                      % (mode, e_t, e_a, cos, e_f, worst_n, worst_s, worst_name))
        if mode != "torch":
            assert max(e_t, e_a) <= 2e-2 and cos >= 0.9998, report[-1]
            assert e_f <= 2e-2, report[-1]
            assert worst_n <= 2e-2 and worst_s <= 5e-2, report[-1]
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "deep_text_audio_parity_report.txt"), "w").write(
        "\n".join(report) + "\n")


@pytest.mark.parametrize("flat,drop_path,recompute", [(False, 0.0, False), (True, 0.0, True), (True, 0.3, False), (False, 0.3, True)])
def test_lock_step_pass_matches_one_forward_per_modality(flat, drop_path, recompute):
    """TransformerEncoder.forward_multi: the text, image and audio streams of a tri-modal step advanced layer by layer in lock-step
    on one packed activation matrix (shared attention-branch GEMMs / LayerNorms once over all rows, grouped launches for the narrow
    FFN GEMMs) against one forward per modality (the reference's call pattern, image_text_pretrain_loss.py:76-105):
    the embeddings and the loss must be BIT-IDENTICAL (per row the same kernels do the same arithmetic), so must every gradient of
    the per-modality parameters (FFN sets, adapters' own weights are reached through bit-identical input gradients); the gradients
    of the modality-SHARED parameters are one fp32 sum over all rows instead of three sums rounded to bf16 and added -- equal within
    bf16 rounding (stated deviation, closer to fp32).  flat: gradients accumulated in place in FlatParameters (merged weight-gradient
    launches); drop_path: the same per-sample drop-path draws in both runs; recompute: checkpoint_activations (layer activations
    recomputed in backward) or kept."""
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=3, attention_heads=2, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B = 6
    inp = _to_dev(synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000))
    L = cfg["layers"]
    g = torch.Generator(device="cpu").manual_seed(5)
    table = (torch.bernoulli(torch.full((L, 2, 3 * B), 0.7), generator=g) / 0.7).to(DEV)  # fixed per-sample drop-path multipliers
    calls = {"n": 0}
    orig = TE.TransformerEncoder._draw_path_scales

    def fixed_draw(self, nb, device):
        if drop_path <= 0.0:
            return None
        o = 0 if nb == 3 * B else calls["n"] * B   # lock-step: all samples at once; separate passes: text, image, audio in turn
        calls["n"] += 1
        return [(table[i, 0, o:o + nb], table[i, 1, o:o + nb]) for i in range(L)]
    TE.TransformerEncoder._draw_path_scales = fixed_draw
    res = {}
    try:
        for lock in (False, True):
            enc = one_peace_encoder_config(drop_path_rate=drop_path, layer_scale_init_value=1e-2, checkpoint_activations=recompute, **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(torch.bfloat16).train()
            fl = FlatParameters(m) if flat else None
            calls["n"] = 0
            used = {"multi": 0}
            if lock:
                orig_multi = TE.TransformerEncoder.forward_multi

                def counted(self, infos):
                    used["multi"] += 1
                    return orig_multi(self, infos)
                TE.TransformerEncoder.forward_multi = counted
            try:
                loss, _, log = TriModalContrastiveCriterion(None, 0.0, lock_step=lock)(m, {"net_input": inp, "nsentences": B})
                if fl is not None:
                    fl.zero_grad()
                else:
                    m.zero_grad()
                loss.backward()
                torch.cuda.synchronize()
            finally:
                if lock:
                    TE.TransformerEncoder.forward_multi = orig_multi
            assert used["multi"] == (1 if lock else 0)
            res[lock] = (float(loss.detach()), {n: q.grad.detach().float().clone() for n, q in m.named_parameters() if q.grad is not None})
    finally:
        TE.TransformerEncoder._draw_path_scales = orig
    assert res[True][0] == res[False][0], (res[True][0], res[False][0])
    shared_tags = ("self_attn.", "self_attn_layer_norm", "final_layer_norm", "gamma_1", "gamma_2", "logit_scale")
    n_exact = n_close = 0
    for n, gs in res[False][1].items():
        gm = res[True][1][n]
        if any(t in n for t in shared_tags):
            assert float((gm - gs).norm()) <= 2e-2 * float(gs.norm()) + 1e-5, (n, float((gm - gs).norm()), float(gs.norm()))
            n_close += 1
        else:
            assert torch.equal(gm, gs), (n, float((gm - gs).abs().max()))
            n_exact += 1
    assert n_exact > 40 and n_close > 20


def test_fused_encoder_returns_all_hiddens_and_honours_layerdrop(golden_dir):
    """TransformerEncoder on the HIP path with the two switches that used to send a pass to the torch ops (VERDICT r4 missing #4):
    return_all_hiddens (transformer_encoder.py:186-199: every executed layer's output per modality, T x B x C) and layerdrop in training
    (fairseq/modules/layer_drop.py:13-44; transformer_encoder.py:48-51).  (Round 6) Against what the UNMODIFIED REFERENCE returned for
    the same weights, inputs and seed of the CPU generator (tests/golden/layerdrop_hiddens.pt, make_golden.py layerdrop_fixture): the
    fused path must run exactly the layers the reference ran -- counted -- and return its states and encoder output within the
    activation bound (1.5e-2), for a joint text+image stream and a text-only stream, eval and training."""
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from one_peace_amd.transformer import transformer_layer as TL
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    fx = _fx(golden_dir, "layerdrop_hiddens.pt")
    enc = one_peace_encoder_config(drop_path_rate=0.0, checkpoint_activations=False, **fx["cfg"])
    enc.layerdrop = fx["layerdrop"]
    torch.manual_seed(0)
    m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(fx["vocab"]), "val"), fx["shapes"])
    m = m.to(DEV).to(torch.bfloat16)
    W = m.encoder_wrapper
    inp = _to_dev(fx["inputs"])
    fused_calls = {"n": 0}
    orig_fused = TL.TransformerEncoderLayer.forward_fused

    def counted(self, *a, **k):
        fused_calls["n"] += 1
        return orig_fused(self, *a, **k)
    TL.TransformerEncoderLayer.forward_fused = counted
    report = []
    try:
        for case in fx["cases"]:
            m.train(case["train"])
            n_run = sum(case["ran"])
            with torch.no_grad():
                t = W.text_adapter(inp["src_tokens"], None, None, None)
                i = W.image_adapter(inp["src_images"], None, None, None, False)
                for et, infos in (("vl", (t, i, None)), ("text", (t, None, None))):
                    fused_calls["n"] = 0
                    torch.manual_seed(case["seed"])  # the layerdrop mask comes from the CPU generator, once per pass
                    out = W.fusion_model(*infos, return_all_hiddens=True, encoder_type=et)
                    assert fused_calls["n"] == n_run, (case["train"], case["seed"], et, fused_calls["n"], n_run)
                    want = case[et]
                    assert len(out["text_encoder_states"]) == n_run and out["audio_encoder_states"] == []
                    assert len(out["image_encoder_states"]) == (n_run if et == "vl" else 0)
                    pairs = [("out", out["encoder_out"][0], want["encoder_out"])]
                    pairs += [("text state %d" % k, a, b) for k, (a, b) in enumerate(zip(out["text_encoder_states"], want["text_states"]))]
                    pairs += [("image state %d" % k, a, b) for k, (a, b) in enumerate(zip(out["image_encoder_states"], want["image_states"]))]
                    for what, got, ref in pairs:
                        assert got.shape == ref.shape, (what, got.shape, ref.shape)
                        e = rel_fro(got.float().cpu(), ref)
                        report.append("train %d seed %2d %-4s %-14s %.3e" % (case["train"], case["seed"], et, what, e))
                        assert e <= 1.5e-2, (case["seed"], et, what, e)
    finally:
        TL.TransformerEncoderLayer.forward_fused = orig_fused
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "layerdrop_hiddens_parity_report.txt"), "w").write(
        "\n".join(report) + "\n")


@pytest.mark.parametrize("lock,recompute", [(False, False), (True, False), (True, True)])
def test_layer_scale_gradient_from_the_weight_gradient_matches_the_branch_output_form(lock, recompute):
    """ops.dgamma_from_wgrad_ok (round 5): with flat gradients and whole 256 x 256 weight-gradient tiles the residual GEMMs write no
    branch output y; gamma_1 / gamma_2 get their gradient from the out-proj / down-projection weight gradients (row dot of W with the
    launch's UNSCALED fp32 product, + bias * g0; round 6: no division).  Against the y form of the same code
    (ONEPEACE_DGAMMA_FROM_WGRAD=0): the same loss; every gradient within bf16 rounding of the y form AND of the plain-autograd
    (non-flat) run -- since round 6 the branch gradient travels without gamma (gamma sits in the weight-gradient epilogue and in the
    transposed weight copy of the input gradient), so the two forms round at different places and are no longer bit-identical
    upstream of the residual; less memory held."""
    from one_peace_amd import ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=256, ffn_embed_dim=512, layers=3, attention_heads=4, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B = 64  # every stream's row count (and their sum) a multiple of 64: the weight gradients ride on the grouped launch
    inp = _to_dev(synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000))
    res = {}
    old = ops.DGAMMA_FROM_WGRAD
    fused_seen = {"n": 0}
    orig_ok = ops.dgamma_from_wgrad_ok

    def counted_ok(*a, **k):
        r = orig_ok(*a, **k)
        fused_seen["n"] += int(bool(r))
        return r
    ops.dgamma_from_wgrad_ok = counted_ok
    try:
        for mode in ("autograd", "y", "wgrad"):
            ops.DGAMMA_FROM_WGRAD = mode == "wgrad"
            enc = one_peace_encoder_config(drop_path_rate=0.0, layer_scale_init_value=1e-1, checkpoint_activations=recompute, **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(torch.bfloat16).train()
            fl = FlatParameters(m) if mode != "autograd" else None
            (fl or m).zero_grad()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            fused_seen["n"] = 0
            loss, _, _ = TriModalContrastiveCriterion(None, 0.0, lock_step=lock)(m, {"net_input": inp, "nsentences": B})
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated() - base
            loss.backward()
            torch.cuda.synchronize()
            res[mode] = (float(loss.detach()), held, fused_seen["n"],
                         {n: q.grad.detach().float().clone() for n, q in m.named_parameters() if q.grad is not None})
            del m, fl, loss
    finally:
        ops.DGAMMA_FROM_WGRAD = old
        ops.dgamma_from_wgrad_ok = orig_ok
    assert res["wgrad"][2] >= 6 and res["y"][2] == 0, (res["wgrad"][2], res["y"][2])  # every branch of every layer took the new form
    assert res["wgrad"][0] == res["y"][0]
    n_gamma = 0
    for n, g in res["y"][3].items():
        gw = res["wgrad"][3][n]
        if n.endswith("gamma_1") or n.endswith("gamma_2"):
            n_gamma += 1
            ga = res["autograd"][3][n]
            assert rel_fro(gw, ga) <= 2e-2 and rel_fro(g, ga) <= 2e-2, (n, rel_fro(gw, ga), rel_fro(g, ga))
            assert rel_fro(gw, g) <= 2e-2, (n, rel_fro(gw, g))
        else:  # gamma * (u^T x) against (gamma u)^T x, u (gamma W)^T against (gamma u) W^T: one bf16 rounding placed differently
            ga = res["autograd"][3].get(n)
            if ga is None:  # a parameter the step does not use (mask embeddings): no gradient under autograd, zeros in the flat buffer
                assert float(g.abs().max()) == 0.0 and float(gw.abs().max()) == 0.0, n
                continue
            assert rel_fro(gw, g) <= 2e-2, (n, rel_fro(gw, g))  # (measured up to 1.3e-2 at these micro dimensions)
            assert rel_fro(gw, ga) <= max(2e-2, 1.5 * rel_fro(g, ga)), (n, rel_fro(gw, ga), rel_fro(g, ga))
    assert n_gamma == 6
    if not recompute:
        assert res["wgrad"][1] < res["y"][1], (res["wgrad"][1], res["y"][1])  # 4 H of the 46 H bytes per token and layer are not kept


@pytest.mark.parametrize("lock,fp8", [(False, False), (True, False), (False, True), (True, True)])
def test_recompute_cheap_level_gives_the_same_bits_with_less_kept_memory(lock, fp8):
    """ops.set_recompute_cheap: the memory level between "keep everything" and checkpoint_activations -- the four
    LayerNorm-type outputs only weight gradients read (LN1(x), the attention sub-LayerNorm's output, LN2(x_mid), LN_F(gelu(h0) h1))
    are re-created in backward by the same kernels on the same kept rows.  Loss and EVERY gradient must be bit-identical to the
    keep-everything run, and less memory must be held between forward and backward.  lock: the lock-step pass (AttnBranchFn and
    FfnBranchMultiFn over all rows) or one pass per modality (both with one row segment).  fp8 (round 6): with the opt-in fp8
    forward FFN the level used to be ignored silently for the FFN branch (bench.py's memory estimate assumed it); backward reads the
    bf16 rows, which the plain kernels re-create bit for bit next to what the _q8 variants wrote in the forward."""
    from one_peace_amd import ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=256, ffn_embed_dim=512, layers=3, attention_heads=4, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)  # F % 256 == 0: the split GeGLU form, whose LN_F output the cheap level drops
    B = 6
    inp = _to_dev(synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000))
    res = {}
    old = ops.set_recompute_cheap(False)
    old_fp8 = ops.set_fp8_ffn(fp8)
    try:
        for cheap in (False, True):
            ops.set_recompute_cheap(cheap)
            enc = one_peace_encoder_config(drop_path_rate=0.0, layer_scale_init_value=1e-1, checkpoint_activations=False, **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(torch.bfloat16).train()
            fl = FlatParameters(m)
            fl.zero_grad()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            loss, _, _ = TriModalContrastiveCriterion(None, 0.0, lock_step=lock)(m, {"net_input": inp, "nsentences": B})
            torch.cuda.synchronize()
            held = torch.cuda.memory_allocated() - base
            loss.backward()
            torch.cuda.synchronize()
            res[cheap] = (float(loss.detach()), held, {n: q.grad.detach().clone() for n, q in m.named_parameters() if q.grad is not None})
            del m, fl, loss
    finally:
        ops.set_recompute_cheap(old)
        ops.set_fp8_ffn(old_fp8)
    assert res[True][0] == res[False][0]
    assert len(res[True][2]) == len(res[False][2]) > 60
    for n, g in res[False][2].items():  # (the relative-position tables too: their gradient is summed in a fixed order)
        assert torch.equal(res[True][2][n], g), (n, float((res[True][2][n].float() - g.float()).abs().max()))
    # per token and layer LN1(x), the sub-LayerNorm output, LN2(x) (2 H bytes each) and LN_F(GeGLU) (2 F = 4 H bytes here) are not kept:
    # 10 H bytes x layers x rows (text 16 + image 17 tokens per sample, + the audio frames) -- at the 4B dimensions (F = 4 H) 14 of 46 H
    saved = res[False][1] - res[True][1]
    assert saved >= 0.9 * 10 * cfg["embed_dim"] * cfg["layers"] * B * (16 + 17), (res[True][1], res[False][1])


def _skip_dropped_runs(flat, recompute, variants):
    """Loss, gradients and the number of op_rows_gather calls of one lock-step tri-modal step under fixed stochastic-depth masks, per
    variant (skip_dropped_branches, ops.SKIP_ROW_TABLES).  The masks include a layer without drop-path, a branch that keeps every
    sample, one that drops a whole modality (multiplier fallback for that branch) and one that keeps a single sample of a segment."""
    from one_peace_amd import hip as hipm, ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=4, attention_heads=2, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B, L, rate = 6, 4, 0.45
    inp = _to_dev(synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000))
    probs = torch.linspace(0, rate, L).tolist()
    g = torch.Generator(device="cpu").manual_seed(11)
    mask = torch.bernoulli(torch.full((L, 2, 3 * B), 0.6), generator=g).bool()
    mask[1, 0] = True                    # a branch that keeps everything
    mask[2, 0, :B] = False               # ... that drops the whole text segment (samples 0..B-1): multiplier fallback
    mask[3, 1, B:2 * B] = False
    mask[3, 1, B + 2] = True             # ... that keeps one image sample
    orig_scales, orig_mask, orig_tables = TE.TransformerEncoder._draw_path_scales, TE.TransformerEncoder._draw_keep_mask, ops.SKIP_ROW_TABLES

    def fixed_scales(self, nb, device):
        assert nb == 3 * B
        return [(None, None) if p <= 0.0 else ((mask[i, 0].float() / (1 - p)).to(device), (mask[i, 1].float() / (1 - p)).to(device))
                for i, p in enumerate(probs)]
    TE.TransformerEncoder._draw_path_scales = fixed_scales
    TE.TransformerEncoder._draw_keep_mask = staticmethod(lambda pr, n: mask.clone())
    res = {}
    try:
        for skip, tables in variants:
            ops.SKIP_ROW_TABLES = tables
            enc = one_peace_encoder_config(drop_path_rate=rate, layer_scale_init_value=1e-1, checkpoint_activations=recompute, **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(torch.bfloat16).train()
            m.encoder_wrapper.fusion_model.skip_dropped_branches = skip
            fl = FlatParameters(m) if flat else None
            packed = {"n": 0}
            orig_gather = hipm.rows_gather

            def counted(src, kr):
                packed["n"] += 1
                return orig_gather(src, kr)
            hipm.rows_gather = counted
            try:
                loss, _, log = TriModalContrastiveCriterion(None, 0.0, lock_step=True)(m, {"net_input": inp, "nsentences": B})
                (fl.zero_grad() if fl is not None else m.zero_grad())
                loss.backward()
                torch.cuda.synchronize()
            finally:
                hipm.rows_gather = orig_gather
            res[(skip, tables)] = (float(loss.detach()), {n: q.grad.detach().float().clone() for n, q in m.named_parameters() if q.grad is not None},
                                   packed["n"])
    finally:
        TE.TransformerEncoder._draw_path_scales, TE.TransformerEncoder._draw_keep_mask, ops.SKIP_ROW_TABLES = orig_scales, orig_mask, orig_tables
    return res


@pytest.mark.parametrize("flat,recompute", [(False, False), (True, False), (True, True)])
def test_lock_step_pass_that_skips_dropped_samples_matches_the_multiplier_form(flat, recompute):
    """TransformerEncoder.skip_dropped_branches: every residual branch of the lock-step pass is computed for the samples stochastic
    depth KEEPS only (hip.KeptRows; round 6: read and written through the row table) instead of for all samples with the dropped ones
    multiplied by zero (transformer_layer.py:78-88).  Same masks in both runs: the loss and every gradient must agree within bf16
    rounding (the packed GEMMs see other row counts, so tile shapes / split-K may differ; weight gradients sum the same non-zero terms
    in another order)."""
    res = _skip_dropped_runs(flat, recompute, [(False, True), (True, True)])
    ref, got = res[(False, True)], res[(True, True)]
    assert ref[2] == 0 and got[2] == 0, (ref[2], got[2])  # no packed copies any more
    assert abs(got[0] - ref[0]) <= 2e-3 * abs(ref[0]), (got[0], ref[0])
    assert set(got[1]) == set(ref[1])
    for n, gd in ref[1].items():
        e = float((got[1][n] - gd).norm()) / (float(gd.norm()) + 1e-6)
        assert e <= 3e-2, (n, e)
    assert len(got[1]) > 60, len(got[1])


@pytest.mark.parametrize("flat,recompute", [(False, False), (True, False), (True, True)])
def test_row_tables_give_the_bits_of_the_packed_copies(flat, recompute):
    """(round 6, ABI 9) The same step with ops.SKIP_ROW_TABLES on (LayerNorm forward / backward, op_resid_bwd and the residual epilogue
    read and write the full matrix through hip.KeptRows.rowmap) and off (round 4: op_rows_gather in front of, op_rows_merge behind every
    packed branch, forward and backward): the same loss and the same gradients BIT FOR BIT -- except the bias tables, whose gradient sums
    fp32 atomics in either form."""
    res = _skip_dropped_runs(flat, recompute, [(True, False), (True, True)])
    old, new = res[(True, False)], res[(True, True)]
    # 3 layers with drop-path x 2 branches, minus the fallback branch: 5 packed branches, each gathered in forward and backward
    assert old[2] == 10 and new[2] == 0, (old[2], new[2])
    assert old[0] == new[0], (old[0], new[0])
    assert set(old[1]) == set(new[1])
    for n, gd in old[1].items():
        if "rel_pos_table" in n:
            assert float((new[1][n] - gd).norm()) <= 1e-3 * float(gd.norm()) + 1e-6, n
        else:
            assert torch.equal(new[1][n], gd), (n, float((new[1][n] - gd).abs().max()))


def test_skipped_branches_against_the_fp32_oracle_under_the_same_masks():
    """skip_dropped_branches against the ORACLE (round-4 verdict: it had only been compared with the multiplier form of the same
    HIP code): the fp32 CPU oracle runs the three towers with the SAME host-drawn drop-path masks (transformer_layer.py:78-88,
    `path_scales` = per layer one [B] multiplier vector per residual branch) -- loss, per-modality features and every parameter
    gradient of BOTH forms are held to it at the common bounds (features 1.5e-2, gradients 5e-2 + 1.5e-3 absolute).

    And the two HIP forms against each other: per row the packed form performs the multiplier form's arithmetic (a kept sample's
    branch rows go through the same LayerNorm / GEMM K-loops / attention items / residual epilogue, a dropped sample's rows are
    passed through where the multiplier form adds 0 * branch), so the FORWARD features of all samples must be bit-identical and with
    them the loss.  Parameter gradients are not bit-identical: a weight gradient is a sum over rows, the packed launch sums the
    kept rows only (other K extents, other tile / split-K partitions) while the multiplier form sums all rows with exact zeros in
    between -- the same terms in another order, rounded to bf16 once; both are gated against the oracle at the common bound."""
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=4, attention_heads=2, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B, L, rate = 6, 4, 0.45
    raw = synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000)
    inp = _to_dev(raw)
    probs = torch.linspace(0, rate, L).tolist()
    g = torch.Generator(device="cpu").manual_seed(23)
    mask = torch.bernoulli(torch.full((L, 2, 3 * B), 0.6), generator=g).bool()
    mask[1, 1] = True                    # a branch that keeps everything
    mask[2, 1, 2 * B:] = False
    mask[2, 1, 2 * B + 1] = True         # ... that keeps one audio sample
    for i in range(L):                   # every segment keeps a sample in every branch: all branches with drop-path are PACKED
        for b in range(2):
            for s0 in (0, B, 2 * B):
                if not bool(mask[i, b, s0:s0 + B].any()):
                    mask[i, b, s0] = True
    orig_scales, orig_mask = TE.TransformerEncoder._draw_path_scales, TE.TransformerEncoder._draw_keep_mask

    def fixed_scales(self, nb, device):
        assert nb == 3 * B
        return [(None, None) if p <= 0.0 else ((mask[i, 0].float() / (1 - p)).to(device), (mask[i, 1].float() / (1 - p)).to(device))
                for i, p in enumerate(probs)]
    TE.TransformerEncoder._draw_path_scales = fixed_scales
    TE.TransformerEncoder._draw_keep_mask = staticmethod(lambda pr, n: mask.clone())
    orig_multi = TE.TransformerEncoder.forward_multi
    res, sd_fp32 = {}, None
    try:
        for skip in (False, True):
            enc = one_peace_encoder_config(drop_path_rate=rate, layer_scale_init_value=1e-1, **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(torch.bfloat16).train()
            enc_m = m.encoder_wrapper.fusion_model
            enc_m.skip_dropped_branches = skip
            enc_m.pack_min_drop = (0.0, 0.0)
            feats = {}

            def capture(self, infos):
                out = orig_multi(self, infos)
                feats.update({k: v.detach().clone() for k, v in out.items()})
                return out
            TE.TransformerEncoder.forward_multi = capture
            try:
                loss, _, log = TriModalContrastiveCriterion(None, 0.0, lock_step=True)(m, {"net_input": inp, "nsentences": B})
                m.zero_grad()
                loss.backward()
                torch.cuda.synchronize()
            finally:
                TE.TransformerEncoder.forward_multi = orig_multi
            assert set(feats) == {"text", "image", "audio"}
            if sd_fp32 is None:
                sd_fp32 = {k: (v.detach().float().cpu().requires_grad_(True) if v.is_floating_point() else v.detach().cpu())
                           for k, v in m.state_dict().items()}
            res[skip] = (loss.detach().float().cpu(), {k: v.float().cpu() for k, v in feats.items()},
                         {n: q.grad.detach().float().cpu() for n, q in m.named_parameters() if q.grad is not None})
    finally:
        TE.TransformerEncoder._draw_path_scales, TE.TransformerEncoder._draw_keep_mask = orig_scales, orig_mask
        TE.TransformerEncoder.forward_multi = orig_multi
    # ---- fp32 oracle with the same masks: segment order text, image, audio = sample ranges [0,B), [B,2B), [2B,3B) ----
    heads = cfg["attention_heads"]

    def scales(s0):
        return [None if p <= 0.0 else (mask[i, 0, s0:s0 + B].float() / (1 - p), mask[i, 1, s0:s0 + B].float() / (1 - p))
                for i, p in enumerate(probs)]
    t, ft = O.contrastive_embed(sd_fp32, heads, L, "text", path_scales=scales(0), src_tokens=raw["src_tokens"])
    i_, fi = O.contrastive_embed(sd_fp32, heads, L, "image", path_scales=scales(B), src_images=raw["src_images"].to(torch.bfloat16).float())
    a, fa = O.contrastive_embed(sd_fp32, heads, L, "audio", path_scales=scales(2 * B),
                                src_audios=raw["src_audios"].to(torch.bfloat16).float(), audio_padding_masks=raw["audio_padding_masks"])
    sc = O.logit_scale_exp(sd_fp32["logit_scale"])
    ref = O.itc_loss(i_, t, i_, t, sc)[0] + O.itc_loss(a, t, a, t, sc)[0]
    ref.backward()
    want_feats = {"text": ft.detach(), "image": fi.detach(), "audio": fa.detach()}
    report = []
    for skip in (False, True):
        loss, feats, grads = res[skip]
        tag = "packed" if skip else "multiplier"
        assert abs(float(loss) - float(ref)) <= 2.5e-2, (tag, float(loss), float(ref))
        for mname, want in want_feats.items():
            e = rel_fro(feats[mname], want)
            report.append("%-10s features %-6s %.3e" % (tag, mname, e))
            assert e <= 1.5e-2, (tag, mname, e)
        n = 0
        for name, got in grads.items():
            want = sd_fp32[name].grad
            assert want is not None, name
            err, nw = float((got - want).norm()), float(want.norm())
            report.append("%-10s grad %-70s %.3e (|ref| %.3e)" % (tag, name, err / (nw + 1e-30), nw))
            assert err <= 5e-2 * nw + 1.5e-3, (tag, name, err, nw)
            n += 1
        assert n > 60, n
    # ---- packed form against multiplier form: forward bit-identical (all samples, kept or dropped), so is the loss ----
    for mname in want_feats:
        assert torch.equal(res[True][1][mname], res[False][1][mname]), (mname, float((res[True][1][mname] - res[False][1][mname]).abs().max()))
    assert float(res[True][0]) == float(res[False][0])
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "skip_dropped_oracle_parity_report.txt"), "w").write(
        "\n".join(report) + "\n")


@pytest.mark.parametrize("stage", ["vl", "al"])
def test_pair_criterions_take_a_pretrain_model_in_lock_step(golden_dir, stage):
    """Round-4 advisor finding: OnePeacePretrainModel.forward_multi returns {modality: (logits, features)} tuples where the
    retrieval model returns bare embeddings; the pair criterions (lock-step is their default on the HIP path) must unwrap them as
    the one-call-per-modality branch does: same loss bits either way."""
    from tests.test_model_cpu import _build_pretrain
    from one_peace_amd.criterions.contrastive import AudioTextRetrievalCriterion, ImageTextRetrievalCriterion
    from one_peace_amd.transformer import transformer_encoder as TE
    fx = _fx(golden_dir, "micro_pretrain.pt" if stage == "vl" else "micro_pretrain_al.pt")
    ni = {k: (v.to(DEV).to(torch.bfloat16) if v.is_floating_point() else v.to(DEV)) for k, v in fx["net_input"].items()}
    Crit = ImageTextRetrievalCriterion if stage == "vl" else AudioTextRetrievalCriterion
    m = _build_pretrain(fx, audio_language=stage == "al").to(DEV).to(torch.bfloat16).train()
    used = {"multi": 0}
    orig_multi = TE.TransformerEncoder.forward_multi

    def counted(self, infos):
        used["multi"] += 1
        return orig_multi(self, infos)
    TE.TransformerEncoder.forward_multi = counted
    losses = {}
    try:
        for lock in (True, False):
            m.zero_grad()
            loss, _, log = Crit(None, 0.0, lock_step=lock)(m, {"net_input": ni, "nsentences": ni["src_tokens"].shape[0]})
            loss.backward()
            torch.cuda.synchronize()
            losses[lock] = float(loss.detach())
            assert all(torch.isfinite(q.grad).all() for q in m.parameters() if q.grad is not None)
    finally:
        TE.TransformerEncoder.forward_multi = orig_multi
    assert used["multi"] == 1, used
    assert losses[True] == losses[False], losses


@pytest.mark.parametrize("other", ["image", "audio"])
def test_pair_criterions_in_lock_step_match_one_forward_per_modality(other):
    """image_text_retrieval_criterion / audio_text_retrieval_criterion (BASELINE configs 2 and 4): text + image (audio) advanced in
    lock-step through the shared encoder against one model call per modality (image_text_retrieval_loss.py:64-112): same loss
    bits, per-modality gradients bit-identical, gradients of the shared attention branch within bf16 rounding (one fp32 sum over all
    rows instead of two rounded sums)."""
    from one_peace_amd.criterions.contrastive import AudioTextRetrievalCriterion, ImageTextRetrievalCriterion
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=3, attention_heads=2, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B = 6
    inp = _to_dev(synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000))
    Crit = ImageTextRetrievalCriterion if other == "image" else AudioTextRetrievalCriterion
    res = {}
    for lock in (False, True):
        enc = one_peace_encoder_config(drop_path_rate=0.0, layer_scale_init_value=1e-2, **cfg)
        torch.manual_seed(0)
        m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
        m = m.to(DEV).to(torch.bfloat16).train()
        used = {"multi": 0}
        orig_multi = TE.TransformerEncoder.forward_multi

        def counted(self, infos):
            used["multi"] += 1
            return orig_multi(self, infos)
        TE.TransformerEncoder.forward_multi = counted
        try:
            m.zero_grad()
            loss, _, log = Crit(None, 0.0, lock_step=lock)(m, {"net_input": inp, "nsentences": B})
            loss.backward()
            torch.cuda.synchronize()
        finally:
            TE.TransformerEncoder.forward_multi = orig_multi
        assert used["multi"] == (1 if lock else 0)
        res[lock] = (float(loss.detach()), {n: q.grad.detach().float().clone() for n, q in m.named_parameters() if q.grad is not None})
    assert res[True][0] == res[False][0], (res[True][0], res[False][0])
    shared_tags = ("self_attn.", "self_attn_layer_norm", "final_layer_norm", "gamma_1", "gamma_2", "logit_scale")
    assert set(res[True][1]) == set(res[False][1])
    for n, gs in res[False][1].items():
        gm = res[True][1][n]
        if any(t in n for t in shared_tags):
            assert float((gm - gs).norm()) <= 2e-2 * float(gs.norm()) + 1e-5, (n, float((gm - gs).norm()), float(gs.norm()))
        else:
            assert torch.equal(gm, gs), (n, float((gm - gs).abs().max()))


def test_single_stream_skip_of_dropped_samples_matches_the_multiplier_form():
    """skip_dropped_branches on a SINGLE-modality training pass (image tower, the forwards of BASELINE configs 2 and 4): it runs as a
    lock-step pass with one segment and packs the kept samples of every branch; same masks as the multiplier form -> embeddings
    and gradients within bf16 rounding."""
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=3, attention_heads=2, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B, L, rate = 7, 3, 0.4
    imgs = _to_dev(synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000))["src_images"]
    probs = torch.linspace(0, rate, L).tolist()
    g = torch.Generator(device="cpu").manual_seed(3)
    mask = torch.bernoulli(torch.full((L, 2, B), 0.6), generator=g).bool()
    mask[:, :, 0] = True
    orig_scales, orig_mask = TE.TransformerEncoder._draw_path_scales, TE.TransformerEncoder._draw_keep_mask
    TE.TransformerEncoder._draw_path_scales = lambda self, nb, device: [
        (None, None) if p <= 0.0 else ((mask[i, 0].float() / (1 - p)).to(device), (mask[i, 1].float() / (1 - p)).to(device))
        for i, p in enumerate(probs)]
    TE.TransformerEncoder._draw_keep_mask = staticmethod(lambda pr, n: mask.clone())
    res = {}
    try:
        for skip in (False, True):
            enc = one_peace_encoder_config(drop_path_rate=rate, layer_scale_init_value=1e-1, **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(torch.bfloat16).train()
            m.encoder_wrapper.fusion_model.skip_dropped_branches = skip
            m.zero_grad()
            emb = m(src_images=imgs, encoder_type="image")
            (emb.float() * torch.linspace(-1, 1, emb.numel(), device=DEV).view_as(emb)).sum().backward()
            torch.cuda.synchronize()
            res[skip] = (emb.detach().float().cpu(), {n: q.grad.detach().float().clone() for n, q in m.named_parameters() if q.grad is not None})
    finally:
        TE.TransformerEncoder._draw_path_scales, TE.TransformerEncoder._draw_keep_mask = orig_scales, orig_mask
    assert rel_fro(res[True][0], res[False][0]) <= 1e-2
    assert set(res[True][1]) == set(res[False][1]) and len(res[True][1]) > 25
    for n, gd in res[False][1].items():
        e = float((res[True][1][n] - gd).norm()) / (float(gd.norm()) + 1e-6)
        assert e <= 3e-2, (n, e)


def test_vision_tower_40_layers_matches_reference(golden_dir):
    """tests/golden/deep_vision40.pt: the reference's FULL-DEPTH image tower -- 40 layers at the 4B layer dimensions (1.5 B
    parameters, BASELINE configs[1]) -- one 256^2 image, forward, run on CPU in fp32 through ref_shim.  The HIP path in bf16 against
    it with ABSOLUTE gates (bf16 storage through 40 layers; the 8-layer fixture measures 1.3e-2): normalised CLS embedding
    rel-Frobenius <= 4e-2 and cosine >= 0.9992, probe rows of the final features <= 4e-2, residual-stream norm within 1 %."""
    fx = _fx(golden_dir, "deep_vision40.pt")
    imgs = synth.synth_inputs(1, image_res=fx["image_res"], vocab=fx["vocab"])["src_images"].to(DEV).to(torch.bfloat16)
    m = load_synth(build_retrieval(dict(fx["cfg"]), fx["vocab"], head_type="image")).to(DEV).to(torch.bfloat16).eval()
    assert sum(q.numel() for q in m.state_dict().values()) == fx["nparams"]
    with torch.no_grad():
        logits = m(src_images=imgs, encoder_type="image").float().cpu()
        feats = m.encoder_wrapper(src_images=imgs, encoder_type="image")[1].float().cpu()
    torch.cuda.synchronize()
    del m
    torch.cuda.empty_cache()
    e_l = rel_fro(logits, fx["logits"])
    cos = float(torch.nn.functional.cosine_similarity(logits, fx["logits"], dim=1).min())
    e_f = rel_fro(feats[0, [0, 1, 128, 256]], fx["feats_rows"])
    e_n = abs(float(feats.double().norm()) - float(fx["feats_norm"])) / float(fx["feats_norm"])
    line = "40 layers: logits rel-fro %.3e cos %.6f | probe rows %.3e | feature-norm deviation %.3e" % (e_l, cos, e_f, e_n)
    open(os.path.join(os.path.dirname(os.path.dirname(__file__)), "gpurun_out", "deep_vision40_parity_report.txt"), "w").write(line + "\n")
    assert e_l <= 4e-2 and cos >= 0.9992 and e_f <= 4e-2 and e_n <= 1e-2, line


def test_stage2_pretraining_skips_frozen_weight_gradients(golden_dir):
    """Stage-2 audio-language pretraining (`stage2_pretrain: true`, one_peace_pretrain.py:98-104) on the HIP path against the
    reference-written fixture micro_pretrain_al_stage2.pt: loss, the set of parameters that receive a gradient, those gradients
    -- and the fused backward must not LAUNCH the weight-gradient GEMMs of frozen parameters (counted with the library's launch
    profiler: the same step with everything trainable runs strictly more GEMM launches)."""
    from tests.test_model_cpu import _build_pretrain
    from one_peace_amd.criterions.pretrain import AudioTextPretrainLossCriterion
    from one_peace_amd import hip
    fx = _fx(golden_dir, "micro_pretrain_al_stage2.pt")
    ni = {k: (v.to(DEV).to(torch.bfloat16) if v.is_floating_point() else v.to(DEV)) for k, v in fx["net_input"].items()}
    crit = AudioTextPretrainLossCriterion(None, 1.0, 0.5, 0.5, 2.5, label_smoothing=0.0)
    launches, grads, losses = {}, {}, {}
    for stage2 in (True, False):
        m = _build_pretrain(fx, audio_language=True, stage2=stage2).to(DEV).to(torch.bfloat16).eval()
        loss, _, _ = crit(m, {"net_input": ni, "nsentences": 4})
        m.zero_grad()
        torch.cuda.synchronize()
        hip.lib().op_prof_enable(1)
        loss.backward()
        hip.lib().op_prof_enable(0)
        launches[stage2] = hip.profile_kernels.collect(4)[0]["count"]
        grads[stage2] = {n: q.grad.detach().float().cpu() for n, q in m.named_parameters() if q.grad is not None}
        losses[stage2] = float(loss.detach())
    assert sorted(grads[True]) == fx["with_grad"]
    assert abs(losses[True] - float(fx["loss"])) <= 3e-2 * abs(float(fx["loss"])) and losses[True] == losses[False]
    assert 0 < launches[True] < launches[False], launches
    n = 0
    for k, ref in fx["grads"].items():
        if k.endswith("#norm") or k.endswith("#rows4") or float(ref.norm()) < 1e-7:
            continue
        e = float((grads[True][k] - ref).norm())
        assert e <= 6e-2 * float(ref.norm()) + 2e-2, (k, e, float(ref.norm()))
        # a gradient does not depend on which OTHER parameters are frozen (only the order in which autograd adds the passes'
        # bf16 contributions up may differ)
        assert float((grads[True][k] - grads[False][k]).norm()) <= 1e-2 * float(grads[False][k].norm()) + 1e-6, k
        n += 1
    assert n > 20


@pytest.mark.parametrize("dgrad", [False, True])
def test_fp8_ffn_forward_in_the_lock_step_pass(dgrad):
    """dgrad (round 6): ALSO the two input-gradient GEMMs of the FFN backward (dy W2, dh [W0 | W1]) on e4m3 operands -- gradient rows
    quantised by op_quant_fp8_rows, the transposed weight copies once per optimiser step; the weight gradients stay bf16.
    Round 5: with ops.set_fp8_ffn(True) a TRAINING lock-step pass keeps the lock-step form (it used to fall back to one pass per
    modality): LayerNorm2 / op_ln_geglu_fwd emit the fp8 operands, the plain N = 2F up-projection and the down-projection + residual run
    on the fp8 kernels per modality.  Same loss bits as the fp8 passes taken one by one (per row the same kernels), and within the
    variant's tolerance of the bf16 step; every gradient finite (backward = bf16 kernels on the saved bf16 activations)."""
    from one_peace_amd import ops as _ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from tests.model_util import TinyDictionary
    from types import SimpleNamespace
    cfg = dict(embed_dim=256, ffn_embed_dim=512, layers=2, attention_heads=4, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B = 5
    inp = _to_dev(synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000))
    res = {}
    used = {"multi": 0, "fp8": 0}
    orig_multi, orig_f8 = TE.TransformerEncoder.forward_multi, _ops.hip.gemm_nt_fp8

    def counted(self, infos):
        used["multi"] += 1
        return orig_multi(self, infos)

    def counted_f8(*a, **k):
        used["fp8"] += 1
        return orig_f8(*a, **k)
    for mode in ("bf16", "fp8 lock-step", "fp8 one by one"):
        enc = one_peace_encoder_config(drop_path_rate=0.0, layer_scale_init_value=1e-1, checkpoint_activations=False, **cfg)
        torch.manual_seed(0)
        m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
        m = m.to(DEV).to(torch.bfloat16).train()
        old_dg = _ops.FP8_FFN_DGRAD
        old = _ops.set_fp8_ffn(mode != "bf16", dgrad=dgrad)
        TE.TransformerEncoder.forward_multi, _ops.hip.gemm_nt_fp8 = counted, counted_f8
        used["multi"] = used["fp8"] = 0
        try:
            loss, _, _ = TriModalContrastiveCriterion(None, 0.0, lock_step=mode != "fp8 one by one")(m, {"net_input": inp, "nsentences": B})
            m.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
        finally:
            _ops.set_fp8_ffn(old, dgrad=old_dg)
            TE.TransformerEncoder.forward_multi, _ops.hip.gemm_nt_fp8 = orig_multi, orig_f8
        assert used["multi"] == (0 if mode == "fp8 one by one" else 1), (mode, used)
        # 2 layers x 3 modalities x (up, down [, dy W2, dh W01]); the first layer's FFN input gradient is needed too (adapters train)
        assert used["fp8"] == (0 if mode == "bf16" else 2 * 3 * (4 if dgrad else 2)), (mode, used)
        res[mode] = (float(loss.detach()), {n: q.grad.detach().float().clone() for n, q in m.named_parameters() if q.grad is not None})
    assert res["fp8 lock-step"][0] == res["fp8 one by one"][0], (res["fp8 lock-step"][0], res["fp8 one by one"][0])
    assert abs(res["fp8 lock-step"][0] - res["bf16"][0]) <= 2e-2 * abs(res["bf16"][0]), (res["fp8 lock-step"][0], res["bf16"][0])
    for n, g8 in res["fp8 lock-step"][1].items():
        g16 = res["bf16"][1][n]
        assert g8.isfinite().all(), n
        assert float((g8 - g16).norm()) <= 0.2 * float(g16.norm()) + 2e-3, (n, float((g8 - g16).norm()), float(g16.norm()))


@pytest.mark.parametrize("fp8", [False, True])
def test_train_step_graph_replay_matches_eager_training(fp8):
    """graphs.TrainStepGraph: zero-grad + three forwards + ITC/ATC + the whole backward (custom autograd functions, in-place
    accumulation into the flat gradient buffer, autograd's own accumulation for the adapters) recorded into ONE hipGraph and
    replayed, optimiser step eager in between: losses and parameters must follow eager training bit for bit, also when the
    static batch is overwritten with new data between replays.  fp8: the opt-in e4m3 forward FFN GEMMs -- their quantised weight
    copies are derived buffers a replay reads by address, so the optimiser step has to re-quantise them in place (a
    replay kept reading the step-0 weights)."""
    from one_peace_amd import ops as _ops
    old_fp8 = _ops.set_fp8_ffn(fp8)
    try:
        _graph_vs_eager()
    finally:
        _ops.set_fp8_ffn(old_fp8)


def _graph_vs_eager():
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import BucketedGradReducer, FlatParameters
    from one_peace_amd.graphs import TrainStepGraph
    from one_peace_amd.optim import FusedAdamW
    cfg = dict(embed_dim=128, ffn_embed_dim=256, layers=2, attention_heads=2, image_rel_bucket_size=4,
               text_bucket_size=256, audio_bucket_size=512)
    batches = [_to_dev(synth.synth_inputs(8, text_len=15, image_res=64, audio_samples=8000, vocab=1000, seed=s)) for s in (1, 2)]
    runs = {}
    for mode in ("eager", "graph"):
        m = load_synth(build_retrieval(cfg, 1000)).to(DEV).to(torch.bfloat16).eval()
        flat = FlatParameters(m)
        reducer = BucketedGradReducer(flat)
        opt = FusedAdamW(flat, lr=1e-3)
        crit = TriModalContrastiveCriterion(None, 0.0)
        static = {k: v.clone() for k, v in batches[0].items()}

        def fwd_bwd():
            opt.zero_grad()
            reducer.reset()
            loss, _, _ = crit(m, {"net_input": static, "nsentences": 8})
            loss.backward()
            return loss
        start = flat.params.clone()
        g = None
        if mode == "graph":
            g = TrainStepGraph(fwd_bwd, warmup=1)  # the warm-up / capture passes only touch gradients, never parameters
            assert torch.equal(flat.params, start)
        losses = []
        for i in range(4):
            for k, v in batches[i % 2].items():
                static[k].copy_(v)
            loss = g.replay() if g is not None else fwd_bwd()
            reducer.finish()
            opt.step(clip_norm=3.0)
            losses.append(float(loss.detach()))
        torch.cuda.synchronize()
        runs[mode] = (losses, flat.params.clone())
    assert runs["eager"][0] == runs["graph"][0], (runs["eager"][0], runs["graph"][0])
    assert torch.equal(runs["eager"][1], runs["graph"][1])
    assert len(set(runs["eager"][0])) == 4  # the steps really differ (new data, updated weights)


def test_retrieval_criteria_on_hip(golden_dir):
    """BASELINE configs[2] objective: image_text_retrieval_criterion (ITC, eps 0) and audio_text_retrieval_criterion (ATC with
    label smoothing 0.1, the eps/(n-1) form of image_text_retrieval_loss.py:21-24) through the HIP InfoNCE kernels, against
    the losses and hit counts the reference produced."""
    from one_peace_amd.criterions.contrastive import AudioTextRetrievalCriterion, ImageTextRetrievalCriterion
    fx = _fx(golden_dir, "micro_retrieval.pt")
    m = load_synth(build_retrieval(fx["cfg"], fx["vocab"]), fx["shapes"]).to(DEV).to(torch.bfloat16).eval()
    inp = _to_dev(fx["inputs"])
    sample = {"net_input": inp, "nsentences": 4}
    l_it, _, log_it = ImageTextRetrievalCriterion(None, label_smoothing=0.0)(m, sample)
    l_at, _, log_at = AudioTextRetrievalCriterion(None, label_smoothing=0.1)(m, sample)
    assert abs(float(l_it.detach()) - float(fx["itc_loss"])) < 2e-2 and abs(float(l_at.detach()) - float(fx["atc_loss"])) < 2e-2
    assert float(log_it["i2t_ncorrect"]) == float(fx["i2t"]) and float(log_it["t2i_ncorrect"]) == float(fx["t2i"])
    assert float(log_at["a2t_ncorrect"]) == float(fx["a2t"]) and float(log_at["t2a_ncorrect"]) == float(fx["t2a"])
    (l_it + l_at).backward()
    assert m.logit_scale.grad is not None and torch.isfinite(m.logit_scale.grad)


def test_hub_interface_feature_extraction_on_hip(golden_dir):
    """BASELINE configs[0]/[1] surface on the device: OnePeaceHubInterface(device='cuda', dtype='bf16') and its four
    extract_*_features calls (hub_interface.py:206-225) run the HIP path and reproduce the reference's outputs."""
    from one_peace_amd import hip
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    fx = _fx(golden_dir, "micro_retrieval.pt")
    hub = OnePeaceHubInterface(load_synth(build_retrieval(fx["cfg"], fx["vocab"]), fx["shapes"]), device=DEV, dtype="bf16")
    assert next(hub.model.parameters()).dtype == torch.bfloat16 and not hub.model.training
    inp = fx["inputs"]
    before = hip.GEMM_ALGO_BYTES[1]
    toks = hub.process_text([row[row != 1] for row in inp["src_tokens"]])
    assert torch.equal(toks.cpu(), inp["src_tokens"])
    outs = {"text": hub.extract_text_features(toks),
            "image": hub.extract_image_features(hub.process_image(inp["src_images"])),
            "audio": hub.extract_audio_features(inp["src_audios"].to(DEV), inp["audio_padding_masks"].to(DEV)),
            "vl": hub.extract_vl_features(inp["src_images"].to(DEV), toks)}
    assert hip.GEMM_ALGO_BYTES[1] > before  # the HIP GEMMs ran (no torch fallback)
    refs = {"text": fx["text_logits"], "image": fx["image_logits"], "audio": fx["audio_logits"], "vl": fx["vl_text"][:, 0]}
    for k, ref in refs.items():
        got = outs[k].float().cpu()
        assert got.shape == ref.shape and not outs[k].requires_grad, k
        assert rel_fro(got, ref) < 2e-2, (k, rel_fro(got, ref))


def test_hub_interface_graph_replay_matches_eager(golden_dir):
    """enable_graphs(): each extract_* call captured into one hipGraph per input shape; replay is bit-identical to the eager
    HIP path, follows new input values, and a new batch shape gets its own graph."""
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    fx = _fx(golden_dir, "micro_retrieval.pt")
    hub = OnePeaceHubInterface(load_synth(build_retrieval(fx["cfg"], fx["vocab"]), fx["shapes"]), device=DEV, dtype="bf16")
    inp = _to_dev(fx["inputs"])
    calls = {"text": lambda h, sl: h.extract_text_features(inp["src_tokens"][sl]),
             "image": lambda h, sl: h.extract_image_features(inp["src_images"][sl]),
             "audio": lambda h, sl: h.extract_audio_features(inp["src_audios"][sl], inp["audio_padding_masks"][sl]),
             "vl": lambda h, sl: h.extract_vl_features(inp["src_images"][sl], inp["src_tokens"][sl])}
    eager = {k: (f(hub, slice(0, 4)), f(hub, slice(0, 2)), f(hub, slice(2, 4))) for k, f in calls.items()}
    hub.enable_graphs()
    for k, f in calls.items():
        first = f(hub, slice(0, 4))
        assert torch.equal(first, eager[k][0]), k
        assert torch.equal(f(hub, slice(0, 2)), eager[k][1]), k       # second shape -> second graph
        assert torch.equal(f(hub, slice(2, 4)), eager[k][2]), k       # same graph, new values
        assert torch.equal(f(hub, slice(0, 4)), eager[k][0]), k       # first graph again
        assert torch.equal(first, eager[k][0])                        # returned tensors are not the static buffers
        assert len(hub._graphs[k].graphs) == 2
    hub.enable_graphs(False)
    assert torch.equal(calls["text"](hub, slice(0, 4)), eager["text"][0])
