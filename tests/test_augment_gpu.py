"""Training-time image augmentation on the device: crops, centre crops and flips through op_image_resize_normalize_flip
(csrc/image.hip) and Mixup / CutMix through op_mix_images (csrc/augment.hip), bit for bit.  References: PIL's outputs in
tests/golden/augment.pt and the CPU restatements tests/test_augment_cpu.py pins to PIL and to timm's statements
(imageprep.apply_packed, timm_mix); PIL itself is not needed here."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from one_peace_amd import augment, hip, imageprep, ops
from tests.test_augment_cpu import source_image, timm_mix, timm_mixup_target

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.uint8, torch.float32, torch.bfloat16)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return torch.load(os.path.join(golden_dir, "augment.pt"), weights_only=False)


def _run(packed, dtype):
    return hip.image_resize_normalize(packed, imageprep.CLIP_MEAN, imageprep.CLIP_STD, dtype, DEV)


def _check_all_dtypes(packed, want_u8, what):
    want32 = imageprep.to_tensor_normalize(want_u8)
    got = {dt: _run(packed, dt) for dt in DTYPES}
    torch.cuda.synchronize()
    assert torch.equal(got[torch.uint8].cpu(), want_u8), what
    assert got[torch.float32].dtype == torch.float32 and torch.equal(got[torch.float32].cpu(), want32), what
    assert got[torch.bfloat16].dtype == torch.bfloat16 and torch.equal(got[torch.bfloat16].cpu(), want32.to(torch.bfloat16)), what


# ---- geometry ---------------------------------------------------------------------------------------------------
def test_crops_and_flips_equal_pil_for_every_output_type(fx):
    """Every crop case of the fixture (1 x 1, full image, corner-flush, upscaling, vertical-first and random boxes), one launch per
    size S = 16 (4 column groups), 32 and 48 (12), every second image flipped."""
    by_size = {}
    for (H, W, S, seed, *box), want in zip(fx["crops"].tolist(), fx["crop_outputs"]):
        by_size.setdefault(S, []).append((source_image(H, W, seed), box, want))
    assert {16, 48} <= set(by_size)
    for S, cases in by_size.items():
        flips = [i % 2 == 1 for i in range(len(cases))]
        packed = imageprep.pack_images([c[0] for c in cases], S, crops=[c[1] for c in cases], flips=flips)
        assert packed.desc[:, 10].any() or S == 32  # the vertical-first boxes are in the S = 16 and S = 48 launches
        want = torch.stack([c[2].flip(1) if f else c[2] for c, f in zip(cases, flips)])
        assert torch.equal(imageprep.apply_packed(packed), want)
        _check_all_dtypes(packed, want, ("crops", S))
        flips = [not f for f in flips]  # ... and the other half
        packed = imageprep.pack_images([c[0] for c in cases], S, crops=[c[1] for c in cases], flips=flips)
        _check_all_dtypes(packed, torch.stack([c[2].flip(1) if f else c[2] for c, f in zip(cases, flips)]), ("crops", S, "other half"))


def test_center_crops_and_flips_equal_pil_for_every_output_type(fx):
    by_size = {}
    for (H, W, S, seed), want in zip(fx["centers"].tolist(), fx["center_outputs"]):
        by_size.setdefault(S, []).append((source_image(H, W, seed), want))
    for S, cases in by_size.items():
        flips = [i % 3 == 0 for i in range(len(cases))]
        packed = imageprep.pack_images([c[0] for c in cases], S, center_crop=True, flips=flips)
        want = torch.stack([c[1].flip(1) if f else c[1] for c, f in zip(cases, flips)])
        _check_all_dtypes(packed, want, ("center", S))
        plain = imageprep.pack_images([c[0] for c in cases], S, center_crop=True)  # no flag array at all: the old entry
        assert plain.flip_off is None
        _check_all_dtypes(plain, torch.stack([c[1] for c in cases]), ("center, old entry", S))


def test_mixed_batch_only_some_images_cropped_or_flipped():
    imgs = [source_image(37, 53, 1), source_image(200, 131, 2), source_image(480, 640, 3), source_image(19, 23, 4), source_image(500, 4, 5)]
    full = lambda i: (0, 0, imgs[i].shape[0], imgs[i].shape[1])
    for S in (16, 48):
        crops = [full(0), (150, 100, 50, 31), full(2), (18, 22, 1, 1), (5, 1, 495, 3)]  # uncropped, corner-flush, 1 x 1, vertical-first
        flips = [False, True, True, False, True]
        packed = imageprep.pack_images(imgs, S, crops=crops, flips=flips)
        want = imageprep.apply_packed(packed)
        plain = torch.stack([imageprep.apply_coeffs(i, S) for i in imgs])
        assert torch.equal(want[0], plain[0]) and torch.equal(want[2], plain[2].flip(1))  # the uncropped ones are the plain resize
        _check_all_dtypes(packed, want, ("mixed", S))
        got = ops.preprocess_images(imgs, S, dtype=torch.bfloat16, device=DEV, crops=crops, flips=flips)
        assert got.is_cuda and torch.equal(got.cpu(), imageprep.to_tensor_normalize(want).to(torch.bfloat16))


def _raw(packed, out, dtype_code, flip):
    """The two entries called directly: flip = None runs op_image_resize_normalize, "null" the new entry with a NULL flag array, a
    list the new entry with those flags in device memory."""
    buf = packed.host.to(DEV)
    ws = torch.zeros(max(packed.workspace_bytes, 16), dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    m, s = (ctypes.c_float * 3)(*imageprep.CLIP_MEAN), (ctypes.c_float * 3)(*imageprep.CLIP_STD)
    args = (ctypes.c_void_p(base), packed.src_bytes, ctypes.c_void_p(base + packed.desc_off), packed.desc.ctypes.data_as(ctypes.c_void_p),
            len(packed), ctypes.c_void_p(base + packed.coef_off), packed.coef_count, packed.size, m, s, hip.ptr(out), dtype_code, hip.ptr(ws),
            ws.numel())
    if flip is None:
        rc = hip.lib().op_image_resize_normalize(*args, hip.stream())
    else:
        flags = None if flip == "null" else torch.tensor(flip, dtype=torch.uint8, device=DEV)
        rc = hip.lib().op_image_resize_normalize_flip(*args, hip.ptr(flags), hip.stream())
    torch.cuda.synchronize()
    return rc


def test_old_entry_and_new_entry_with_zero_flags_give_identical_bytes():
    imgs = [source_image(37, 53, 1), source_image(200, 131, 2), source_image(19, 23, 4), source_image(500, 4, 5)]
    for S in (16, 48):
        packed = imageprep.pack_images(imgs, S)
        for dtype, code in ((torch.uint8, hip.DT_U8), (torch.float32, hip.DT_F32), (torch.bfloat16, hip.DT_BF16)):
            shape = (4, S, S, 3) if dtype == torch.uint8 else (4, 3, S, S)
            outs = []
            for flip in (None, "null", [0, 0, 0, 0], [1, 0, 1, 1]):
                out = torch.zeros(shape, dtype=dtype, device=DEV)
                assert _raw(packed, out, code, flip) == 0
                outs.append(out.cpu())
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), (S, dtype)
            w = 2 if dtype == torch.uint8 else 3  # the column axis
            assert torch.equal(outs[3][1], outs[0][1]) and torch.equal(outs[3][[0, 2, 3]], outs[0][[0, 2, 3]].flip(w)), (S, dtype)


def test_train_image_transform_on_the_device_equals_its_cpu_restatement():
    imgs = [source_image(37, 53, 1), source_image(200, 131, 2), source_image(19, 23, 3), source_image(64, 64, 4)]
    got = augment.TrainImageTransform(32, min_scale=0.9, hflip=0.5, generator=torch.Generator().manual_seed(5))(imgs, torch.bfloat16, DEV)
    g = torch.Generator().manual_seed(5)
    boxes = [imageprep.random_resized_crop_params(i.shape[0], i.shape[1], scale=(0.9, 1.0), generator=g) for i in imgs]
    flips = (torch.rand(4, generator=g) < 0.5).tolist()
    want = imageprep.to_tensor_normalize(imageprep.apply_packed(imageprep.pack_images(imgs, 32, pin=False, crops=boxes, flips=flips)))
    assert got.is_cuda and got.dtype == torch.bfloat16 and torch.equal(got.cpu(), want.to(torch.bfloat16))


# ---- Mixup / CutMix ---------------------------------------------------------------------------------------------
def _tables(mode, B, S, seed, mixup_alpha=0.8, cutmix_alpha=1.0):
    np.random.seed(seed)
    return augment.Mixup(mixup_alpha=mixup_alpha, cutmix_alpha=cutmix_alpha, mode=mode)._draw(B, S, S)


CASES = [(mode, B, S) for mode in ("batch", "elem", "pair") for B in (2, 5, 8) for S in (16, 32) if not (mode == "pair" and B == 5)]


@pytest.mark.parametrize("mode,B,S", CASES)
def test_mix_images_in_place_equals_the_torch_statement(mode, B, S):
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(B * S))
    for k, (ma, ca) in enumerate(((0.8, 0.0), (0.0, 1.0), (0.8, 1.0))):
        (kind, lam, oml, box), tlam = _tables(mode, B, S, 7 * B + S + k, ma, ca)
        want = timm_mix(x, mode, (kind, tlam, box.tolist()))
        xd = x.to(DEV)
        got = ops.mix_images(xd, (kind, lam, oml, box), inplace=True)
        assert got is xd and torch.equal(xd.cpu(), want), (mode, B, S, ma, ca)  # fp32, in place, no clone
        again = ops.mix_images(x.to(DEV), (kind, lam, oml, box), inplace=True)
        assert torch.equal(again, xd)  # two runs are identical
        got16 = ops.mix_images(x.to(DEV), (kind, lam, oml, box), out_dtype=torch.bfloat16)  # fp32 -> bf16: one rounding
        assert got16.dtype == torch.bfloat16 and torch.equal(got16.cpu(), want.to(torch.bfloat16))
        xb = x.to(torch.bfloat16)  # bf16 -> bf16: the fp32 statement on the widened values, rounded once
        want_b = timm_mix(xb.float(), mode, (kind, tlam, box.tolist()))
        xbd = xb.to(DEV)
        assert ops.mix_images(xbd, (kind, lam, oml, box), inplace=True) is xbd and torch.equal(xbd.cpu(), want_b.to(torch.bfloat16))
        got32 = ops.mix_images(xb.to(DEV), (kind, lam, oml, box), out_dtype=torch.float32)  # bf16 -> fp32: exact
        assert got32.dtype == torch.float32 and torch.equal(got32.cpu(), want_b)


def test_mixup_differs_from_an_fma_evaluation_on_these_inputs():
    """The comparison above can tell the two roundings apart: an fp64 (= fma-like) evaluation of the same Mixup differs somewhere."""
    x = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(1))
    (kind, lam, oml, box), tlam = _tables("elem", 8, 32, 3, 0.8, 0.0)
    l, o = torch.from_numpy(lam).double().view(8, 1, 1, 1), torch.from_numpy(oml).double().view(8, 1, 1, 1)
    fused = (x.double() * l + x.flip(0).double() * o).float()
    want = timm_mix(x, "elem", (kind, tlam, box.tolist()))
    assert float((fused != want).float().mean()) > 0.05
    assert torch.equal(ops.mix_images(x.to(DEV), (kind, lam, oml, box)).cpu(), want)


def test_cutmix_boxes_off_the_vector_grid():
    B, S = 6, 16
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(9))
    kind = np.full(B, 2, dtype=np.int32)
    box = np.array([(2, 11, 3, 13),    # xl, xh not multiples of 8
                    (4, 4, 3, 13),     # empty (no rows)
                    (0, S, 0, S),      # the full image
                    (7, 8, 9, 10),     # a single pixel
                    (5, 16, 13, 3),    # empty (xh < xl)
                    (1, 15, 7, 9)], dtype=np.int32)  # straddles the 8-element boundary
    lam, oml = np.ones(B, dtype=np.float32), np.zeros(B, dtype=np.float32)
    want = timm_mix(x, "elem", (kind, lam, [tuple(b) if b[3] >= b[2] else (0, 0, 0, 0) for b in box.tolist()]))
    assert torch.equal(want[2], x[3]) and torch.equal(want[1], x[1]) and int((want[3] != x[3]).sum()) == 3
    for dtype in (torch.float32, torch.bfloat16):
        xd = x.to(dtype).to(DEV)
        ops.mix_images(xd, (kind, lam, oml, box), inplace=True)
        assert torch.equal(xd.cpu(), want.to(dtype)), dtype  # (a copy of bf16-rounded values: the same selection)


def test_out_of_place_leaves_x_and_the_guard_words_untouched():
    B, S = 5, 16
    n = B * 3 * S * S
    x = torch.randn(B, 3, S, S, generator=torch.Generator().manual_seed(4))
    (kind, lam, oml, box), tlam = _tables("elem", B, S, 21)
    want = timm_mix(x, "elem", (kind, tlam, box.tolist()))
    tables = hip.mix_tables((kind, lam, oml, box), B, torch.device(DEV))
    for dtype in (torch.float32, torch.bfloat16):
        xd = x.to(DEV)
        buf = torch.full((64 + n + 64,), -777.0, dtype=dtype, device=DEV)
        out = buf[64:64 + n].view(B, 3, S, S)
        assert hip.mix_images(xd, tables, out) is out
        torch.cuda.synchronize()
        assert torch.equal(xd.cpu(), x)
        assert torch.equal(out.cpu(), want.to(dtype))
        assert bool((buf[:64] == -777.0).all()) and bool((buf[64 + n:] == -777.0).all())


def test_unsupported_width_returns_enotsup_without_a_launch_and_ops_falls_back():
    B, H, W = 4, 12, 20  # W % 8 != 0
    x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(6))
    np.random.seed(5)
    (kind, lam, oml, box), tlam = augment.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem")._draw(B, H, W)
    xd = x.to(DEV)
    out = torch.full_like(xd, 5.0)
    k, l, o, b = hip.mix_tables((kind, lam, oml, box), B, torch.device(DEV))
    rc = hip.lib().op_mix_images(hip.ptr(xd), hip.ptr(out), hip.DT_F32, hip.DT_F32, B, 3 * H * W, H, W, hip.ptr(k), hip.ptr(l), hip.ptr(o),
                                 hip.ptr(b), hip.stream())
    torch.cuda.synchronize()
    assert rc == -95 and "not supported" in hip.lib().op_last_error().decode()
    assert bool((out == 5.0).all())  # nothing was launched
    assert hip.mix_images(xd, (k, l, o, b), out) is None
    got = ops.mix_images(xd, (kind, lam, oml, box))
    assert got.is_cuda and torch.equal(got.cpu(), timm_mix(x, "elem", (kind, tlam, box.tolist())))
    # bad arguments are OP_EINVAL, also without a launch
    ok = torch.randn(2, 3, 16, 16, device=DEV)
    k, l, o, b = hip.mix_tables((np.ones(2, np.int32), np.ones(2, np.float32), np.zeros(2, np.float32), np.zeros((2, 4), np.int32)), 2,
                                torch.device(DEV))
    for kw in (dict(in_dtype=7), dict(H=0), dict(CHW=3 * 16 * 16 + 8), dict(B=-1), dict(out_dtype=hip.DT_BF16, alias=True)):
        a = dict(in_dtype=hip.DT_F32, out_dtype=hip.DT_F32, B=2, CHW=3 * 16 * 16, H=16, W=16, alias=False)
        a.update(kw)
        out = torch.full_like(ok, 5.0)
        rc = hip.lib().op_mix_images(hip.ptr(ok), hip.ptr(ok if a["alias"] else out), a["in_dtype"], a["out_dtype"], a["B"], a["CHW"], a["H"],
                                     a["W"], hip.ptr(k), hip.ptr(l), hip.ptr(o), hip.ptr(b), hip.stream())
        torch.cuda.synchronize()
        assert rc == -22 and bool((out == 5.0).all()), kw


# ---- end to end ------------------------------------------------------------------------------------------------
def test_transform_mixup_and_classify_loss_end_to_end(monkeypatch):
    """TrainImageTransform -> Mixup -> ops.classify_loss on device logits [8, 10]: the soft targets take the ROW_LOSS_SOFT route and
    the loss agrees with the torch fallback within the gate tests/test_criteria_gpu.py uses for the loss sum of soft rows (CAP_UNITS
    units per row loss plus the fp32 sum over the rows)."""
    from tests.test_criteria_cpu import SOFT, U, rows_fp64
    from tests.test_criteria_gpu import CAP_UNITS
    imgs = [source_image(20 + 3 * i, 50 - 2 * i, i) for i in range(8)]
    tf = augment.TrainImageTransform(16, min_scale=0.9, hflip=0.5, generator=torch.Generator().manual_seed(1))
    x = tf(imgs, torch.float32, DEV)
    labels = torch.tensor([3, 1, 4, 1, 5, 9, 2, 6], device=DEV)
    np.random.seed(2)
    state = np.random.get_state()
    mix = augment.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=10)
    before = x.clone()
    xm, soft = mix(x, labels)
    assert xm is x and soft.is_cuda and soft.dtype == torch.float32 and tuple(soft.shape) == (8, 10)
    np.random.set_state(state)
    (kind, lam, oml, box), tlam = mix._draw(8, 16, 16)
    assert torch.equal(xm.cpu(), timm_mix(before.cpu(), "elem", (kind, tlam, box.tolist())))
    assert torch.equal(soft.cpu(), timm_mixup_target(labels.cpu(), 10, torch.from_numpy(tlam).unsqueeze(1), 0.1))
    logits = (xm.reshape(8, -1)[:, :10] * 3.0).contiguous().requires_grad_(True)  # device logits [8, 10]
    modes = []
    real = hip.row_loss
    monkeypatch.setattr(hip, "row_loss", lambda xx, tt, mode, *a, **kw: (modes.append(mode), real(xx, tt, mode, *a, **kw))[1])
    loss, n_correct = ops.classify_loss(logits, soft)
    loss.backward()
    assert modes == [hip.ROW_LOSS_SOFT]
    ref_logits = logits.detach().cpu().requires_grad_(True)
    ref_loss, ref_correct = ops.classify_loss(ref_logits, soft.cpu())  # CPU tensors: the reference's torch statements
    l64, c64, g64, lscale, gscale = rows_fp64(SOFT, ref_logits.detach(), soft.cpu())
    gate = CAP_UNITS * (U * float(lscale.sum()) + 8 * 10 * 2.0 ** -126) + (1 + math.ceil(math.log2(8))) * U * float(l64.abs().sum())
    print("end to end: loss %.7f, torch fallback %.7f, fp64 %.7f, gate %.3e" % (float(loss), float(ref_loss), float(l64.sum()), gate))
    assert abs(float(loss) - float(ref_loss)) <= gate
    assert abs(float(loss) - float(l64.sum())) <= gate
