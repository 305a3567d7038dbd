"""op_image_resize_normalize on the device (csrc/image.hip): PIL's bicubic resize + torchvision's ToTensor / Normalize, bit for bit
against tests/golden/preprocess.pt (PIL's uint8 outputs; the fp32 / bf16 references follow from them by torchvision's arithmetic on
the CPU).  Reads only the fixture: neither PIL nor the reference is needed here, except for the file-path test."""
import ctypes
import os

import pytest
import torch

from one_peace_amd import hip, imageprep
from tests.model_util import build_retrieval, load_synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def source_image(H, W, seed):  # = tests/golden/make_preprocess_golden.py: source_image
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return torch.load(os.path.join(golden_dir, "preprocess.pt"), weights_only=False)


def _by_size(fx):
    groups = {}
    for (H, W, S, seed, _), want in zip(fx["cases"].tolist(), fx["outputs"]):
        groups.setdefault(S, []).append((source_image(H, W, seed), want))
    return groups


def _run(images, S, dtype):
    packed = imageprep.pack_images(images, S)
    return hip.image_resize_normalize(packed, imageprep.CLIP_MEAN, imageprep.CLIP_STD, dtype, DEV)


def test_uint8_output_equals_pil_on_every_case(fx):
    for S, cases in _by_size(fx).items():
        for src, want in cases:  # one image per launch
            assert torch.equal(_run([src], S, torch.uint8)[0].cpu(), want), (tuple(src.shape), S)


def test_mixed_batches_equal_the_torchvision_reference_bit_for_bit(fx):
    for S, cases in _by_size(fx).items():
        srcs = [c[0] for c in cases]
        want_u8 = torch.stack([c[1] for c in cases])
        want32 = imageprep.to_tensor_normalize(want_u8)
        got_u8 = _run(srcs, S, torch.uint8)
        got32 = _run(srcs, S, torch.float32)
        got16 = _run(srcs, S, torch.bfloat16)
        torch.cuda.synchronize()
        assert torch.equal(got_u8.cpu(), want_u8), S
        assert got32.dtype == torch.float32 and torch.equal(got32.cpu(), want32), S
        assert got16.dtype == torch.bfloat16 and torch.equal(got16.cpu(), want32.to(torch.bfloat16)), S


def test_batch_order_and_repeat_runs_are_bit_identical(fx):
    cases = _by_size(fx)[48]
    srcs = [c[0] for c in cases]
    first = _run(srcs, 48, torch.bfloat16)
    again = _run(srcs, 48, torch.bfloat16)
    assert torch.equal(first, again)
    perm = torch.randperm(len(srcs), generator=torch.Generator().manual_seed(3)).tolist()
    shuffled = _run([srcs[i] for i in perm], 48, torch.bfloat16)
    assert torch.equal(shuffled, first[perm])


def _raw_call(packed, S, desc, out, ws_bytes=None, src_bytes=None):
    """op_image_resize_normalize on a packed batch with a (possibly corrupted) descriptor table in both memories."""
    buf = packed.host.to(DEV)
    dbytes = torch.from_numpy(desc.view("uint8").reshape(-1)).to(DEV)
    buf[packed.desc_off:packed.desc_off + dbytes.numel()] = dbytes
    ws = torch.zeros(max(packed.workspace_bytes, 16), dtype=torch.uint8, device=DEV)
    base = buf.data_ptr()
    m = (ctypes.c_float * 3)(*imageprep.CLIP_MEAN)
    s = (ctypes.c_float * 3)(*imageprep.CLIP_STD)
    rc = hip.lib().op_image_resize_normalize(
        ctypes.c_void_p(base), packed.src_bytes if src_bytes is None else src_bytes, ctypes.c_void_p(base + packed.desc_off),
        desc.ctypes.data_as(ctypes.c_void_p), len(packed), ctypes.c_void_p(base + packed.coef_off), packed.coef_count, S, m, s,
        hip.ptr(out), hip.DT_F32, hip.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, hip.stream())
    torch.cuda.synchronize()
    return rc, hip.lib().op_last_error().decode()


def test_invalid_sizes_are_refused_without_a_launch():
    packed = imageprep.pack_images([source_image(30, 40, 1), source_image(7, 9, 2)], 32)
    out = torch.full((2, 3, 32, 32), 7.0, device=DEV)
    rc, _ = _raw_call(packed, 32, packed.desc.copy(), out)
    assert rc == 0 and not torch.equal(out, torch.full_like(out, 7.0))  # the valid call runs
    bad = []
    for S in (40, 8, 1040):  # S not a multiple of 16 / out of range
        bad.append((S, packed.desc.copy(), {}, "S ="))
    for field in (1, 2):  # H or W equal to 0
        d = packed.desc.copy()
        d[1, field] = 0
        bad.append((32, d, {}, "need H, W >= 1"))
    bad.append((32, packed.desc.copy(), {"src_bytes": packed.src_bytes - 16}, "overrun src"))   # image buffer too small
    bad.append((32, packed.desc.copy(), {"ws_bytes": packed.workspace_bytes - 1}, "workspace"))  # intermediate too small
    d = packed.desc.copy()
    d[0, 4] = 4096  # records longer than the coefficient buffer
    bad.append((32, d, {}, "coefficient"))
    for S, d, kw, msg in bad:
        out.fill_(7.0)
        rc, err = _raw_call(packed, S, d, out, **kw)
        assert rc == -22 and msg in err, (S, kw, err)
        assert torch.equal(out, torch.full_like(out, 7.0)), (S, kw)  # nothing was launched


def _micro_hub(golden_dir):
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    mfx = torch.load(os.path.join(golden_dir, "micro_retrieval.pt"), weights_only=False)
    return OnePeaceHubInterface(load_synth(build_retrieval(mfx["cfg"], mfx["vocab"]), mfx["shapes"]), device=DEV, dtype="bf16")


def _micro(fx):
    rows = [(i, r) for i, r in enumerate(fx["cases"].tolist()) if r[4]]
    return [source_image(H, W, seed) for _, (H, W, S, seed, _) in rows], torch.stack([fx["outputs"][i] for i, _ in rows])


def test_hub_extract_image_features_from_arrays_end_to_end(golden_dir, fx):
    hub = _micro_hub(golden_dir)
    srcs, want_u8 = _micro(fx)
    ref = imageprep.to_tensor_normalize(want_u8)
    images, widths, heights = hub.process_image([s.numpy() for s in srcs], return_image_sizes=True)
    assert images.is_cuda and images.dtype == torch.bfloat16 and torch.equal(images.cpu(), ref.to(torch.bfloat16))
    assert widths.tolist() == [s.shape[1] for s in srcs] and heights.tolist() == [s.shape[0] for s in srcs]
    got = hub.extract_image_features(images)
    want = hub.extract_image_features(hub.process_image(ref))  # the reference's path: fp32 tensor to the device, cast there
    assert torch.equal(got, want)
    assert torch.equal(hub.process_image(srcs), images)  # uint8 tensors


def test_hub_extract_image_features_from_files_end_to_end(golden_dir, fx, tmp_path):
    Image = pytest.importorskip("PIL.Image")
    hub = _micro_hub(golden_dir)
    srcs, want_u8 = _micro(fx)
    paths = []
    for i, s in enumerate(srcs):
        paths.append(str(tmp_path / ("img%d.png" % i)))
        Image.fromarray(s.numpy()).save(paths[-1])
    ref = imageprep.to_tensor_normalize(want_u8)
    got = hub.extract_image_features(hub.process_image(paths))
    assert torch.equal(got, hub.extract_image_features(hub.process_image(ref)))
