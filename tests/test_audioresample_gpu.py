"""op_audio_resample on the device (csrc/audioresample.hip) against the fp64 oracle of tests/audioresample_ref.py, and its hand-over to
op_audio_normalize_pad inside OnePeaceHubInterface.process_audio(resample=True).

The gate is derived, not measured: with S[n] = L sum_j |x[j] h[n M - j L]|, a kernel that rounds each coefficient L h once, forms the
channel mean and the int16 scale with at most one rounding and runs T fused multiply-adds in any order satisfies
|y - y64| <= (T + 3) 2^-24 S[n] for every element."""
import ctypes
import os
import wave

import numpy as np
import pytest
import torch

from one_peace_amd import audioprep, hip, ops
from tests import audioprep_util as U
from tests import audioresample_ref as R
from tests.model_util import build_retrieval, load_synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000, 96000]
FORMATS = [(1, True), (2, True), (1, False), (2, False)]  # (channels, int16)


def _run(clips, rates):
    wavs, lengths = ops.resample_audio(clips, rates, device=DEV)
    torch.cuda.synchronize()
    assert wavs.is_cuda and wavs.dtype == torch.float32
    return wavs.cpu(), lengths.tolist()


def _check(wavs, lengths, clips, rates, what):
    """Every element of every clip against the bound; exact zeros behind each clip."""
    assert wavs.shape == (len(clips), max(lengths))
    worst = 0.0
    for i, (clip, rate) in enumerate(zip(clips, rates)):
        n = lengths[i]
        assert int((wavs[i, n:] != 0).sum()) == 0, "%s: clip %d is not zero behind its %d samples" % (what, i, n)
        if rate == 16000:
            assert n == clip.shape[0] and np.array_equal(wavs[i, :n].numpy(), R.mono64(clip).astype(np.float32)), (what, i)
            continue
        y64, S = R.oracle(clip, rate)
        assert n == y64.shape[0] == R.out_frames(clip.shape[0], rate), (what, i)
        ratio = R.worst_ratio(wavs[i, :n].numpy(), y64, R.bound(S, rate))
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s: clip %d %s %s at %d Hz: error %.3f x the bound" % (what, i, clip.dtype, clip.shape, rate, ratio)
    print("%s: %d clips, worst error / bound %.4f" % (what, len(clips), worst))


@pytest.mark.parametrize("rate", RATES)
def test_every_element_is_within_the_bound(rate):
    lengths = [1, 2, 3, R.taps(rate) - 1, 441, 442, 4409, 4411, 10007]
    clips = []
    for k, n in enumerate(lengths):
        for f, (ch, int16) in enumerate(FORMATS):
            clips += [R.noise(rate + 16 * k + f, n, ch, int16), R.constant(n, ch, int16)]
    wavs, got = _run(clips, [rate] * len(clips))
    _check(wavs, got, clips, [rate] * len(clips), "%d Hz" % rate)


def _mixed():
    clips = [R.noise(101, 7001, 2, True), R.noise(102, 3000, 1, False), R.noise(103, 9999, 1, True), R.noise(104, 5000, 2, False),
             R.noise(105, 12345, 2, True), R.noise(106, 2500, 1, True), R.noise(107, 777, 2, False), R.noise(108, 300, 1, False)]
    return clips, [44100, 16000, 48000, 11025, 22050, 16000, 8000, 44100]


def test_mixed_batch_of_five_rates_and_pass_through_is_repeatable_and_batch_independent():
    clips, rates = _mixed()
    wavs, lengths = _run(clips, rates)
    _check(wavs, lengths, clips, rates, "mixed batch")
    again, _ = _run(clips, rates)
    assert torch.equal(wavs.view(torch.int32), again.view(torch.int32))  # run to run
    rev, _ = _run(clips[::-1], rates[::-1])
    for i in range(len(clips)):
        alone, n = _run([clips[i]], [rates[i]])
        assert n == [lengths[i]] and torch.equal(alone[0].view(torch.int32), wavs[i, : n[0]].view(torch.int32)), i
        assert torch.equal(alone[0].view(torch.int32), rev[len(clips) - 1 - i, : n[0]].view(torch.int32)), i


def test_index_arithmetic_past_2_to_the_31():
    """13.5 M frames at 44.1 kHz: n M reaches 4 897 959 x 441 = 2.16e9."""
    n = 13_500_000
    clip = R.noise(201, n, 1, True)
    wavs, lengths = _run([clip], [44100])
    n_out = 4_897_960
    assert lengths == [n_out] and wavs.shape == (1, n_out) and (n_out - 1) * 441 > 2 ** 31
    rows = np.unique(np.concatenate([np.arange(2048), np.arange(n_out - 2048, n_out), np.arange(0, n_out, 997)]))
    y64, S = R.oracle(clip, 44100, rows=rows)
    ratio = R.worst_ratio(wavs[0].numpy()[rows], y64, R.bound(S, 44100))
    print("13.5 M frames: %d outputs checked, worst error / bound %.4f" % (rows.shape[0], ratio))
    assert ratio <= 1.0
    again, _ = _run([clip], [44100])
    assert torch.equal(wavs.view(torch.int32), again.view(torch.int32))


def _raw_call(packed, desc, out, B=None, src_bytes=None, coef_count=None, out_bytes=None, src_shift=0, out_shift=0):
    buf = packed.host.to(DEV)
    d = np.ascontiguousarray(desc, dtype=np.int64)
    rc = hip.lib().op_audio_resample(
        ctypes.c_void_p(buf.data_ptr() + src_shift), packed.src_bytes if src_bytes is None else src_bytes,
        ctypes.c_void_p(buf.data_ptr() + packed.desc_off), d.ctypes.data_as(ctypes.c_void_p), d.shape[0] if B is None else B,
        ctypes.c_void_p(buf.data_ptr() + packed.coef_off), packed.coef_count if coef_count is None else coef_count,
        ctypes.c_void_p(out.data_ptr() + out_shift), packed.out_bytes if out_bytes is None else out_bytes, hip.stream())
    torch.cuda.synchronize()
    err = hip.lib().op_last_error()
    return rc, err.decode() if err else ""


def test_refusals_are_einval_before_any_launch():
    clips = [R.noise(301, 3000, 1, True), R.noise(302, 500, 2, False)]
    packed = audioprep.pack_resample(clips, [44100, 48000])
    out = torch.empty(2 * packed.rows + 8, device=DEV)  # rows of packed.rows samples, and room for the misaligned-out call
    good = packed.desc

    def desc(row, col, value):
        d = good.copy()
        d[row, col] = value
        return d
    T1 = int(good[1, 6])
    bad = [(desc(0, 1, 0), {}, "frames"), (desc(1, 1, (1 << 27) + 1), {}, "frames"), (desc(0, 2, 3), {}, "channels"),
           (desc(1, 3, 2), {}, "format"), (good, {"src_shift": 8}, "aligned"), (good, {"out_shift": 4}, "aligned"),
           (good, {"src_bytes": 3000 * 2 - 16}, "overruns src"), (desc(1, 0, int(good[1, 0]) + 8), {}, "overruns src"),
           (desc(0, 4, 641), {}, "ratio"), (desc(0, 4, 0), {}, "ratio"), (desc(1, 5, 0), {}, "ratio"), (desc(1, 6, T1 + 1), {}, "taps"),
           (desc(1, 7, 0), {}, "half"), (desc(1, 5, 100), {}, "window"), (desc(0, 8, 2), {}, "coef"),
           (good, {"coef_count": packed.coef_count - 1}, "coef"), (desc(0, 9, int(good[0, 9]) + 1), {}, "out_frames"),
           (desc(1, 9, int(good[1, 9]) - 1), {}, "out_frames"), (desc(1, 10, int(good[1, 10]) + 8), {}, "overruns out"),
           (good, {"out_bytes": int(good[1, 10]) + 4 * int(good[1, 9]) - 4}, "overruns out"), (good, {"B": 65536}, "B =")]
    for d, kw, msg in bad:
        out.fill_(7.0)
        rc, err = _raw_call(packed, d, out, **kw)
        assert rc == -22 and msg in err, (kw, msg, rc, err)
        assert torch.equal(out, torch.full_like(out, 7.0)), (kw, msg)  # nothing was launched
    rc, err = _raw_call(packed, good, out)
    assert rc == 0, err
    n0, n1, rows = int(good[0, 9]), int(good[1, 9]), packed.rows
    assert int((out[n0:rows] != 7.0).sum()) == 0 and int((out[rows + n1:] != 7.0).sum()) == 0  # nothing is written past a clip's samples
    assert int((out[:n0] == 7.0).sum()) == 0 and int((out[rows:rows + n1] == 7.0).sum()) == 0


def _write_wav(path, pcm, rate):
    a = np.asarray(pcm)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if a.ndim == 1 else a.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(a.astype("<i2").tobytes())
    return str(path)


def _micro_hub(golden_dir, device, dtype):
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    mfx = torch.load(os.path.join(golden_dir, "micro_retrieval.pt"), weights_only=False)
    return OnePeaceHubInterface(load_synth(build_retrieval(mfx["cfg"], mfx["vocab"]), mfx["shapes"]), device=device, dtype=dtype), mfx


def test_hub_chain_resample_then_normalise_on_the_device(golden_dir, tmp_path):
    """hub.process_audio(resample=True) = the fp64 normalise oracle (tests/audioprep_util.py) of the kernel's OWN fp32 resampled clips,
    cropped, tiled and padded, within that oracle's bound: offsets, descriptors and the device-to-device hand-over.  The filter's
    arithmetic is gated above."""
    hub, mfx = _micro_hub(golden_dir, DEV, "float32")
    long48 = R.noise(401, 48000 * 16, 2, True) // 4      # 256 000 samples at 16 kHz: cropped to 240 000
    short44 = R.noise(402, 20000, 1, True) // 2           # 7 257 samples: tiled up to 16 000
    mid22 = R.noise(403, 40001, 2, False) * 0.5 + 0.1     # 29 026 samples
    same16 = R.noise(404, 17000, 2, True) // 3            # no resampling: normalised from the staged int16 source
    same16f = R.noise(405, 5000, 1, False)
    path = _write_wav(tmp_path / "s44.wav", short44, 44100)
    wavs, masks = hub.process_audio([(long48, 48000), path, (mid22, 22050), same16, (same16f, 16000)], resample=True)
    torch.cuda.synchronize()
    assert wavs.is_cuda and wavs.dtype == torch.float32 and wavs.shape == (5, 240000)
    res, res_len = _run([long48, short44, mid22], [48000, 44100, 22050])
    assert res_len == [256000, 7257, 29026]
    x32 = [res[0, :256000], res[1, :7257], res[2, :29026], U.mono32(torch.from_numpy(same16)), torch.from_numpy(same16f)]
    lens = [240000, 16000, 29026, 17000, 16000]
    out = wavs.cpu()
    for i, x in enumerate(x32):
        y64, m, r = U.oracle64(x, 240000, 16000)
        assert y64.numel() == lens[i]
        ratio = U.worst_ratio(out[i, : lens[i]], y64, U.bound(y64, m, r))
        assert ratio <= 1.0, "clip %d: error %.3f x the bound" % (i, ratio)
        assert int((out[i, lens[i]:] != 0).sum()) == 0
        f = hub._frames(lens[i]) + 1
        assert not masks[i, :f].any() and masks[i, f:].all()
    plain, plain_masks = hub.process_audio([same16, same16f])  # clips at 16 kHz: the same bits as without resampling
    assert torch.equal(plain[0, :17000], wavs[3, :17000]) and torch.equal(plain[1, :16000], wavs[4, :16000])
    bf_hub, _ = _micro_hub(golden_dir, DEV, "bf16")
    bf, bf_masks = bf_hub.process_audio([(long48, 48000), path, (mid22, 22050), same16, (same16f, 16000)], resample=True)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf_masks, masks)
    feats = bf_hub.extract_audio_features(bf, bf_masks)
    assert feats.shape == (5, mfx["cfg"]["embed_dim"]) and bool(torch.isfinite(feats.float()).all())
