"""Image pre-processing of the hub (hub_interface.py:94-101, 150-204) on the CPU: the fixed-point filter tables of
imageprep.bicubic_coeffs reproduce PIL's bicubic resize bit for bit (tests/golden/preprocess.pt, and random shapes against PIL
itself when it imports), and OnePeaceHubInterface.process_image takes file paths, PIL images and uint8 arrays."""
import os

import numpy as np
import pytest
import torch

from one_peace_amd import imageprep
from tests.model_util import build_retrieval, load_synth


def source_image(H, W, seed):  # = tests/golden/make_preprocess_golden.py: source_image
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return torch.load(os.path.join(golden_dir, "preprocess.pt"), weights_only=False)


def _hub(golden_dir):
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    mfx = torch.load(os.path.join(golden_dir, "micro_retrieval.pt"), weights_only=False)
    return OnePeaceHubInterface(load_synth(build_retrieval(mfx["cfg"], mfx["vocab"]), mfx["shapes"]), device="cpu", dtype="float32")


def _micro(fx):
    rows = [(i, r) for i, r in enumerate(fx["cases"].tolist()) if r[4]]
    return [source_image(H, W, seed) for _, (H, W, S, seed, _) in rows], torch.stack([fx["outputs"][i] for i, _ in rows])


def test_fixture_is_small_and_covers_the_shapes(fx):
    shapes = {(H, W) for H, W, S, _, _ in fx["cases"].tolist()}
    for hw in [(1, 1), (3, 5), (17, 255), (255, 17), (257, 300), (480, 640), (1, 1000), (2000, 37), (1000, 5)]:
        assert hw in shapes
    assert any(imageprep.vertical_first(H, W, S) for H, W, S, _, _ in fx["cases"].tolist())
    sizes = [S for _, _, S, _, _ in fx["cases"].tolist()]
    assert {16, 48, 64, 256, 384} <= set(sizes) and sizes.count(256) == 2 and sizes.count(384) == 1
    assert any(H == W == S for H, W, S, _, _ in fx["cases"].tolist())  # identity
    assert os.path.getsize(os.path.join(os.path.dirname(imageprep.__file__), "..", "tests", "golden", "preprocess.pt")) < 1 << 20


def test_coeffs_apply_equal_pil_on_the_fixture(fx):
    for (H, W, S, seed, _), want in zip(fx["cases"].tolist(), fx["outputs"]):
        got = imageprep.apply_coeffs(source_image(H, W, seed), S)
        assert torch.equal(got, want), (H, W, S)


def test_coeffs_follow_pillow_rules():
    xmin, taps, w = imageprep.bicubic_coeffs(640, 256)  # downscale 2.5: support 5, ksize 2 * 5 + 1
    assert w.shape == (256, 11) and xmin[0] == 0 and taps.max() <= 11
    assert (w.sum(1) >= (1 << 22) - 11).all() and (w.sum(1) <= (1 << 22) + 11).all()  # normalised, each weight rounded once
    xmin, taps, w = imageprep.bicubic_coeffs(256, 256)  # identity: one weight of exactly 2^22 per output
    assert ((w == 1 << 22).sum(1) == 1).all() and ((w != 0).sum(1) == 1).all()
    assert imageprep.bicubic_coeffs(4000, 256)[2].shape[1] == 65  # 12 MP photo: 65-tap horizontal filter
    assert int(imageprep.bicubic_coeffs(1, 16)[1].max()) == 1


def test_coeffs_apply_equal_pil_on_random_shapes():
    Image = pytest.importorskip("PIL.Image")
    g = torch.Generator().manual_seed(7)
    for _ in range(200):
        H, W = (int(v) for v in torch.randint(1, 400, (2,), generator=g))
        S = int(torch.randint(1, 24, (1,), generator=g)) * 16
        img = torch.randint(0, 256, (H, W, 3), generator=g, dtype=torch.uint8)
        want = np.array(Image.fromarray(img.numpy()).resize((S, S), Image.BICUBIC))
        assert np.array_equal(imageprep.apply_coeffs(img, S).numpy(), want), (H, W, S)


def test_pack_images_layout():
    imgs = [source_image(480, 640, 1), source_image(3, 5, 2)]
    p = imageprep.pack_images(imgs, 48, pin=False)
    buf = p.host.numpy()
    assert len(p) == 2 and p.sizes == [(640, 480), (5, 3)]
    for i, im in enumerate(imgs):
        off, H, W, cx, kx, cy, ky, tmp, row0, rows, vfirst = (int(v) for v in p.desc[i])
        assert vfirst == 0
        assert off % 16 == 0 and (H, W) == im.shape[:2] and np.array_equal(buf[off:off + H * W * 3], im.numpy().reshape(-1))
        assert off + H * W * 3 + imageprep.SRC_SLACK <= p.src_bytes and kx % 4 == 0 and ky % 4 == 0 and tmp % 16 == 0
        coef = buf[p.coef_off:].view(np.int32)
        xmin, taps, w = imageprep.bicubic_coeffs(W, 48)
        rec = coef[cx:cx + 48 * (4 + kx)].reshape(48, 4 + kx)
        assert np.array_equal(rec[:, 0], xmin) and np.array_equal(rec[:, 1], taps) and np.array_equal(rec[:, 4:4 + w.shape[1]], w)
        ymin, ytaps, _ = imageprep.bicubic_coeffs(H, 48)
        assert row0 == ymin[0] and row0 + rows == ymin[-1] + ytaps[-1] <= H
    assert np.array_equal(buf[p.desc_off:p.desc_off + p.desc.nbytes].view(np.int64).reshape(p.desc.shape), p.desc)
    assert p.workspace_bytes == sum(imageprep._align(int(r) * 48 * 3) for r in p.desc[:, 9])
    tall = imageprep.pack_images([source_image(1000, 5, 3)], 48, pin=False)  # vertical pass first: [S, W, 3] intermediate
    assert tall.desc[0, 8:].tolist() == [0, 48, 1] and tall.workspace_bytes == imageprep._align(48 * 5 * 3)
    for bad in ([torch.zeros(0, 4, 3, dtype=torch.uint8)], [torch.zeros(4, 4, 3)], [torch.zeros(4, 4, 4, dtype=torch.uint8)]):
        with pytest.raises(ValueError):
            imageprep.pack_images(bad, 48, pin=False)
    for S in (8, 40, 1040):
        with pytest.raises(ValueError):
            imageprep.pack_images(imgs, S, pin=False)


def test_hub_process_image_on_arrays_matches_the_fixture(golden_dir, fx):
    """uint8 arrays / tensors and a uint8 batch give torchvision's normalised tensor of PIL's resize, at the model's own S."""
    hub = _hub(golden_dir)
    assert hub.patch_image_size == imageprep_micro_size()
    srcs, want_u8 = _micro(fx)
    want = imageprep.to_tensor_normalize(want_u8)
    got, widths, heights = hub.process_image([s.numpy() for s in srcs], return_image_sizes=True)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert widths.tolist() == [s.shape[1] for s in srcs] and heights.tolist() == [s.shape[0] for s in srcs]
    assert torch.equal(hub.process_image(srcs), want)
    same = [source_image(64, 64, 5), source_image(64, 64, 6)]
    assert torch.equal(hub.process_image(torch.stack(same)), hub.process_image(same))


def test_hub_process_image_on_files_and_pil_images(golden_dir, fx, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    hub = _hub(golden_dir)
    srcs, want_u8 = _micro(fx)
    want = imageprep.to_tensor_normalize(want_u8)
    paths = []
    for i, s in enumerate(srcs):
        paths.append(str(tmp_path / ("img%d.png" % i)))
        Image.fromarray(s.numpy()).save(paths[-1])
    got, widths, heights = hub.process_image(paths, return_image_sizes=True)
    assert torch.equal(got, want)
    assert widths.tolist() == [s.shape[1] for s in srcs] and heights.tolist() == [s.shape[0] for s in srcs]
    assert torch.equal(hub.process_image([Image.fromarray(s.numpy()) for s in srcs]), want)
    gray = Image.fromarray(srcs[0].numpy()).convert("L")  # converted to RGB, as the reference's .convert("RGB")
    assert torch.equal(hub.process_image([gray]), hub.process_image([np.array(gray.convert("RGB"))]))


def test_hub_process_image_keeps_float_tensors():
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    hub = OnePeaceHubInterface.__new__(OnePeaceHubInterface)
    hub.device, hub.dtype = "cpu", torch.float32
    x = torch.randn(2, 3, 64, 64)
    assert torch.equal(hub.process_image(x), x)
    hub.dtype = torch.bfloat16
    assert torch.equal(hub.process_image(x), x.to(torch.bfloat16))
    assert torch.equal(hub.process_image(x.numpy()), x.to(torch.bfloat16))


def test_hub_process_image_text_pairs(golden_dir, fx):
    hub = _hub(golden_dir)
    srcs, _ = _micro(fx)
    texts = [torch.tensor([0, 5, 6, 2]), torch.tensor([0, 7, 2]), torch.tensor([0, 8, 9, 10, 2]), torch.tensor([0, 2])]
    pairs = list(zip([s.numpy() for s in srcs], texts))
    images, tokens = hub.process_image_text_pairs(pairs)
    assert torch.equal(images, hub.process_image([s.numpy() for s in srcs])) and torch.equal(tokens, hub.process_text(texts))
    (images, widths, heights), tokens = hub.process_image_text_pairs(pairs, return_image_sizes=True)
    assert torch.equal(images, hub.process_image([s.numpy() for s in srcs])) and torch.equal(tokens, hub.process_text(texts))
    assert widths.tolist() == [s.shape[1] for s in srcs] and heights.tolist() == [s.shape[0] for s in srcs]


def imageprep_micro_size():
    return 64  # tests/golden/make_preprocess_golden.py: MICRO_SIZE (image_rel_bucket_size 4 x 16)
