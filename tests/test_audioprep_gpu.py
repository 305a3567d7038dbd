"""op_audio_normalize_pad on the device (csrc/audioprep.hip) through the C-ABI: channel mean, layer norm over the whole clip, crop, tiling,
zero padding and the cast, against the fp64 oracle that tests/test_audioprep_cpu.py ties to the reference's outputs.

The gate is derived, not measured: a kernel that rounds correctly computed m and r to fp32 and evaluates one subtraction and one
multiplication per sample satisfies |y - y64| <= B = 2^-24 (4 |y64| + 2 |m| r) for every element (one rounding each for m, r, the
difference and the product, plus the cancellation term |m| r), and |y_bf16 - y64| <= 2^-8 (|y64| + B) + B after the cast."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

from one_peace_amd import audioprep, hip, ops
from tests import audioprep_util as U
from tests.model_util import build_retrieval, load_synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float32, torch.bfloat16]


@pytest.fixture(scope="module")
def fx(golden_dir):
    return U.load_fixture(golden_dir)


def _run(clips, max_len, min_len, dtype):
    packed = audioprep.pack_clips([c.numpy() if torch.is_tensor(c) else c for c in clips], max_len, min_len)
    out = hip.audio_normalize_pad(packed, dtype, DEV)
    torch.cuda.synchronize()
    return out.cpu(), packed.lengths


def _check_batch(clips, max_len, min_len, dtype, what):
    """Every element of every clip against the fp64 oracle, exact zeros behind each clip, tiled samples equal to their period."""
    out, lengths = _run(clips, max_len, min_len, dtype)
    assert out.dtype == dtype and out.shape == (len(clips), max(lengths))
    worst = 0.0
    for i, clip in enumerate(clips):
        y64, m, r = U.oracle64(U.mono32(clip), max_len, min_len)
        L = y64.numel()
        assert L == lengths[i]
        limit = U.bound(y64, m, r) if dtype == torch.float32 else U.bound_bf16(y64, m, r)
        ratio = U.worst_ratio(out[i, :L].float(), y64, limit)
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s: clip %d %s %s: error %.3f x the bound" % (what, i, clip.dtype, tuple(clip.shape), ratio)
        assert int((out[i, L:].float() != 0).sum()) == 0, "%s: clip %d is not zero behind its %d samples" % (what, i, L)
        n = min(clip.shape[0], max_len)
        if n < L:
            assert torch.equal(out[i, :L], out[i, :n][torch.arange(L) % n]), "%s: clip %d: tiled samples differ from their period" % (what, i)
    print("%s %s: %d clips, T %d, worst error / bound %.3f" % (what, dtype, len(clips), out.shape[1], worst))
    return out


def _real_size_batches():
    s = U.RATE
    crop = [U.source_clip(31, 16 * s, 1, U.FMT_S16, U.NOISE, 0.01, 0.3), U.source_clip(32, 60 * s, 2, U.FMT_F32, U.NOISE, -0.02, 0.2),
            U.source_clip(33, 3 * s // 10, 2, U.FMT_S16, U.TRIANGLE, 0.0, 0.5), U.source_clip(34, 60 * s, 1, U.FMT_S16, U.TRIANGLE, 0.0, 0.9),
            U.source_clip(35, 16 * s, 1, U.FMT_F32, U.NOISE, 0.5, 1e-3), U.source_clip(36, 3 * s // 10, 1, U.FMT_F32, U.NOISE, 0.0, 0.1)]
    odd = [U.source_clip(41, 50001, 1, U.FMT_S16, U.NOISE, 0.0, 0.3), U.source_clip(42, 123457, 1, U.FMT_F32, U.NOISE, 0.1, 0.2),
           U.source_clip(43, 4803, 2, U.FMT_F32, U.TRIANGLE, 0.0, 0.5), U.source_clip(44, 99999, 2, U.FMT_S16, U.NOISE, 0.0, 0.4),
           U.source_clip(45, 16000, 1, U.FMT_S16, U.FULL_SCALE, 0.0, 1.0), U.source_clip(46, 123455, 1, U.FMT_S16, U.NOISE, -0.2, 0.1)]
    return crop, odd


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_numerical_gate_on_the_fixture_cases_and_their_cross_product(fx, dtype):
    for md in (1, 2):
        clips = [c[0] for c in U.fixture_cases(fx) if c[1] == md] + U.cross_product(md)
        _check_batch(clips, U.RATE * md, U.RATE, dtype, "max_seconds %d" % md)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_numerical_gate_at_real_sizes(dtype):
    crop, odd = _real_size_batches()
    out = _check_batch(crop, 15 * U.RATE, U.RATE, dtype, "15 s crop from 16 s and 60 s, 1 s tiling from 0.3 s")
    assert out.shape[1] == 15 * U.RATE
    out = _check_batch(odd, 15 * U.RATE, U.RATE, dtype, "mixed lengths, odd T")
    assert out.shape[1] == 123457


def test_fixture_outputs_are_within_the_reference_s_error_plus_the_bound(fx):
    """Closeness to the reference's actual output follows by the triangle inequality; checked here on the stored outputs."""
    ref_ratio = float(fx["ref_err_over_B"].max())
    for clip, md, want, _ in U.fixture_cases(fx):
        out, _ = _run([clip], U.RATE * md, U.RATE, torch.float32)
        y64, m, r = U.oracle64(U.mono32(clip), U.RATE * md, U.RATE)
        assert U.worst_ratio(out[0], want.double(), U.bound(y64, m, r)) <= ref_ratio + 1.0


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_a_clip_does_not_depend_on_its_batch(dtype):
    _, odd = _real_size_batches()
    max_len, min_len = 15 * U.RATE, U.RATE
    batch, lengths = _run(odd, max_len, min_len, dtype)
    again, _ = _run(odd, max_len, min_len, dtype)
    assert torch.equal(batch.view(torch.int16 if dtype == torch.bfloat16 else torch.int32),
                       again.view(torch.int16 if dtype == torch.bfloat16 else torch.int32))  # run to run
    rev, _ = _run(odd[::-1], max_len, min_len, dtype)
    for i, clip in enumerate(odd):
        alone, _ = _run([clip], max_len, min_len, dtype)
        L = lengths[i]
        assert alone.shape == (1, L)
        assert torch.equal(alone[0], batch[i, :L]) and torch.equal(alone[0], rev[len(odd) - 1 - i, :L]), i


def test_int16_and_the_same_samples_as_fp32_meet_the_same_oracle():
    """s / 32768 is exact, so both sources have the same y64.  The int16 statistics are integer sums and the fp32 ones fp64 sums:
    equal before the rounding to fp32 up to fp64 rounding, so the results are gated, not compared bit for bit."""
    clips = [U.source_clip(51, n, 1, U.FMT_S16, kind, dc, amp) for n, kind, dc, amp in
             ((7, U.NOISE, 0.0, 0.5), (16001, U.NOISE, 0.3, 0.01), (100000, U.TRIANGLE, 0.0, 0.8), (40000, U.FULL_SCALE, 0.0, 1.0))]
    both = clips + [c.float() / 32768.0 for c in clips]
    out = _check_batch(both, 15 * U.RATE, U.RATE, torch.float32, "int16 and the same samples as fp32")
    k = len(clips)
    for i in range(k):
        y64, m, r = U.oracle64(U.mono32(clips[i]), 15 * U.RATE, U.RATE)
        assert U.worst_ratio(out[i, : y64.numel()], out[k + i, : y64.numel()].double(), U.bound(y64, m, r)) <= 2.0


def _raw_call(packed, desc, out, ws, B=None, max_len=None, min_len=None, T=None, out_dtype=hip.DT_F32, src_bytes=None, src_shift=0,
              out_shift=0, ws_shift=0):
    buf = packed.host.to(DEV)
    d = np.ascontiguousarray(desc, dtype=np.int64)
    rc = hip.lib().op_audio_normalize_pad(
        ctypes.c_void_p(buf.data_ptr() + src_shift), packed.src_bytes if src_bytes is None else src_bytes,
        ctypes.c_void_p(buf.data_ptr() + packed.desc_off), d.ctypes.data_as(ctypes.c_void_p), len(packed) if B is None else B,
        packed.max_len if max_len is None else max_len, packed.min_len if min_len is None else min_len,
        ctypes.c_void_p(out.data_ptr() + out_shift), out.shape[1] if T is None else T, out_dtype,
        ctypes.c_void_p(ws.data_ptr() + ws_shift), ws.numel() - ws_shift, hip.stream())
    torch.cuda.synchronize()
    err = hip.lib().op_last_error()
    return rc, err.decode() if err else ""


def test_refusals_are_einval_before_any_launch():
    clips = [U.source_clip(61, 9000, 1, U.FMT_S16, U.NOISE, 0.0, 0.3), U.source_clip(62, 300, 2, U.FMT_F32, U.NOISE, 0.0, 0.3)]
    packed = audioprep.pack_clips([c.numpy() for c in clips], 8000, 1000)
    out = torch.empty(2, packed.T + 8, device=DEV)  # (room for the misaligned-out call)
    ws = torch.empty(packed.workspace_bytes + 64, dtype=torch.uint8, device=DEV)
    good = packed.desc

    def desc(row, col, value):
        d = good.copy()
        d[row, col] = value
        return d
    T = packed.T
    bad = [(desc(0, 1, 0), {}, "frames"), (desc(1, 1, (1 << 27) + 1), {}, "frames"), (desc(0, 2, 3), {}, "channels"),
           (desc(1, 2, 0), {}, "channels"), (desc(1, 3, 2), {}, "format"), (good, {"out_dtype": 5}, "out_dtype"),
           (good, {"src_shift": 8}, "aligned"), (good, {"out_shift": 4}, "aligned"), (good, {"ws_shift": 8}, "aligned"),
           (good, {"src_bytes": 9000 * 2 - 16}, "overruns"), (desc(1, 0, packed.src_bytes), {}, "overruns"),
           (desc(1, 0, int(good[1, 0]) + 8), {}, "overruns"), (good, {"min_len": 9000}, "min_len"), (good, {"max_len": 0}, "max_len"),
           (good, {"B": 65536}, "B ="), (desc(0, 4, 7999), {}, "out_len"), (good, {"T": T - 1}, "out_len"),
           (desc(1, 5, 1), {}, "part_off"), (good, {"ws_shift": packed.workspace_bytes + 48}, "workspace")]
    for d, kw, msg in bad:
        out.fill_(7.0)
        rc, err = _raw_call(packed, d, out, ws, **{"T": T, **kw})
        assert rc == -22 and msg in err, (kw, msg, rc, err)
        assert torch.equal(out, torch.full_like(out, 7.0)), (kw, msg)  # nothing was launched
    rc, err = _raw_call(packed, good, out, ws, T=T)
    assert rc == 0, err


def _write_wav(path, pcm):
    a = np.asarray(pcm)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if a.ndim == 1 else a.shape[1])
        w.setsampwidth(2)
        w.setframerate(U.RATE)
        w.writeframes(a.astype("<i2").tobytes())
    return str(path)


def _micro_hub(golden_dir, device, dtype):
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    mfx = torch.load(os.path.join(golden_dir, "micro_retrieval.pt"), weights_only=False)
    return OnePeaceHubInterface(load_synth(build_retrieval(mfx["cfg"], mfx["vocab"]), mfx["shapes"]), device=device, dtype=dtype), mfx


def test_hub_extract_audio_features_from_files_end_to_end(golden_dir, tmp_path):
    """hub.process_audio(paths) on the device gives the bits of ops.preprocess_audio on the decoded arrays (the numerics are gated at
    the waveform above, so no tolerance here), the CPU route's masks, and finite features of the model's shape."""
    hub, mfx = _micro_hub(golden_dir, DEV, "bf16")
    pcm = [U.source_clip(71, 20001, 1, U.FMT_S16, U.NOISE, 0.0, 0.3), U.source_clip(72, 4000, 2, U.FMT_S16, U.TRIANGLE, 0.05, 0.4),
           U.source_clip(73, 31999, 2, U.FMT_S16, U.NOISE, 0.0, 0.2), U.source_clip(74, 16000, 1, U.FMT_S16, U.TRIANGLE, 0.0, 0.6)]
    paths = [_write_wav(tmp_path / ("clip%d.wav" % i), c.numpy()) for i, c in enumerate(pcm)]
    wavs, masks = hub.process_audio(paths)
    assert wavs.is_cuda and wavs.dtype == torch.bfloat16 and wavs.shape == (4, 31999)
    direct, lengths = ops.preprocess_audio([c.numpy() for c in pcm], U.RATE, 15, 1, dtype=torch.bfloat16, device=DEV)
    assert lengths.tolist() == [20001, 16000, 31999, 16000]
    assert torch.equal(wavs.view(torch.int16), direct.view(torch.int16))
    cpu_hub, _ = _micro_hub(golden_dir, "cpu", "float32")
    cpu_wavs, cpu_masks = cpu_hub.process_audio(paths)
    assert torch.equal(masks.cpu(), cpu_masks) and cpu_wavs.shape == wavs.shape
    feats = hub.extract_audio_features(wavs, masks)
    feats2 = hub.extract_audio_features(direct, cpu_masks.to(DEV))
    assert feats.shape == (4, mfx["cfg"]["embed_dim"]) and bool(torch.isfinite(feats.float()).all())
    assert torch.equal(feats.view(torch.int16), feats2.view(torch.int16))
    mixed, mixed_masks = hub.process_audio([paths[0], pcm[1].numpy(), pcm[2].float() / 32768.0, pcm[3]])  # files, arrays, tensors
    assert torch.equal(mixed_masks, masks) and torch.equal(mixed[[0, 1, 3]].view(torch.int16), wavs[[0, 1, 3]].view(torch.int16))
