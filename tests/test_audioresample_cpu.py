"""Sample-rate conversion on the host (audioprep.resample_filter / resample, ops.resample_audio, ops.preprocess_audio(resample=True),
OnePeaceHubInterface.process_audio(resample=True)) against the fp64 oracle of tests/audioresample_ref.py, which is written from the
filter's definition.  The reference resamples with soxr (librosa.load(sr=16000)); this filter is the project's own, so it is gated by
its closed form and by what a resampler must do to a tone, not by reference outputs.  Needs no GPU."""
import os
import re
import subprocess
import wave

import numpy as np
import pytest
import torch

from one_peace_amd import audioprep, ops
from tests import audioresample_ref as R
from tests.model_util import build_retrieval, load_synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sr_in: (L, M, half), worked out by hand: L / M = 16000 / sr_in, and half = ceil(64 L / fc) = ceil(64 max(L, M) / 0.9475)
SHAPES = {8000: (2, 1, 136), 11025: (640, 441, 43230), 22050: (320, 441, 29788), 24000: (2, 3, 203), 32000: (1, 2, 136),
          44100: (160, 441, 29788), 48000: (1, 3, 203), 88200: (80, 441, 29788), 96000: (1, 6, 406)}


def _hub(golden_dir):
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    mfx = torch.load(golden_dir + "/micro_retrieval.pt", weights_only=False)
    return OnePeaceHubInterface(load_synth(build_retrieval(mfx["cfg"], mfx["vocab"]), mfx["shapes"]), device="cpu", dtype="float32")


def _write_wav(path, pcm, rate):
    a = np.asarray(pcm)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if a.ndim == 1 else a.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(a.astype("<i2").tobytes())
    return str(path)


def test_filter_shape_symmetry_and_refusals():
    assert sorted(SHAPES) == R.RATES
    for rate, (L, M, half) in SHAPES.items():
        gl, gm, h = audioprep.resample_filter(rate)
        assert (gl, gm) == (L, M) and h.dtype == np.float64 and h.shape == (2 * half + 1,), rate
        assert np.array_equal(h, h[::-1]), rate
        rl, rm, rhalf, rh = R.lowpass(rate)
        assert (rl, rm, rhalf) == (L, M, half) and np.abs(h - rh).max() <= 1e-18, rate  # the product's filter is the formula's
        assert abs(h.sum() - 1.0) < 1e-6, rate  # unit gain at 0 Hz: every phase sums to 1 / L
        assert audioprep.resample_length(10007, L, M) == R.out_frames(10007, rate)
    assert audioprep.resample_filter(16000, 8000)[:2] == (1, 2)
    with pytest.raises(ValueError, match=r"L = 16000.*640"):
        audioprep.resample_filter(44101)
    with pytest.raises(ValueError, match=r"L = 3200.*640"):
        audioprep.resample_filter(12345)
    for bad in (0, -44100, 44100.0, 22050.5, True, "44100"):
        with pytest.raises(ValueError, match="positive integer"):
            audioprep.resample_filter(bad)
    with pytest.raises(ValueError, match="positive integer"):
        audioprep.resample_filter(44100, 0)


@pytest.mark.parametrize("rate", [44100, 48000, 22050])
def test_tone_properties_of_the_oracle(rate):
    """A 0.25 s sine below the 7.58 kHz cut-off comes out as the same sine at 16 kHz, one above the 8 kHz Nyquist frequency does not come
    out at all; the central half of the output is clear of the clip's ends (the filter spans 64 / 0.9475 output samples a side)."""
    n = rate // 4
    t_in = np.arange(n, dtype=np.float64) / rate
    n_out = R.out_frames(n, rate)
    rows = np.arange(n_out // 4, n_out - n_out // 4)
    t_out = rows.astype(np.float64) / 16000.0
    for f in (1000.0, 5000.0, 6000.0, 6500.0, 7000.0):
        y, _ = R.oracle(np.sin(2 * np.pi * f * t_in), rate, rows=rows)
        assert np.abs(y - np.sin(2 * np.pi * f * t_out)).max() <= 1e-6, (rate, f)
    for f in (8500.0, 9000.0):
        y, _ = R.oracle(np.sin(2 * np.pi * f * t_in), rate, rows=rows)
        assert np.abs(y).max() < 1e-6, (rate, f)


def test_oracle_is_scipy_resample_poly_with_this_window():
    signal = pytest.importorskip("scipy.signal")
    x = np.random.default_rng(7).standard_normal(700)
    for rate in R.RATES:
        L, M, _, h = R.lowpass(rate)
        y, _ = R.oracle(x, rate)
        want = signal.resample_poly(x, L, M, window=h)
        assert want.shape == y.shape and np.abs(y - want).max() <= 1e-12, rate


def _check_cpu(clip, rate, what):
    wavs, lengths = ops.resample_audio([clip], [rate])
    y64, _ = R.oracle(clip, rate)
    assert wavs.dtype == torch.float32 and wavs.shape == (1, y64.shape[0]) and lengths.tolist() == [y64.shape[0]], what
    err = np.abs(wavs[0].numpy().astype(np.float64) - y64)
    assert (err <= 2.0 ** -24 * np.abs(y64) + 2.0 ** -149).all(), (what, float((err / np.maximum(np.abs(y64), 1e-300)).max()))


@pytest.mark.parametrize("rate", R.RATES)
def test_ops_resample_audio_on_the_cpu_equals_the_oracle_rounded_once(rate):
    n = R.taps(rate) * 3 + 11
    _check_cpu(R.noise(rate, 2 * n, 1, True), rate, "int16 mono")
    _check_cpu(R.noise(rate + 1, n, 2, True), rate, "int16 stereo")
    _check_cpu(R.noise(rate + 2, n, 1, False), rate, "fp32 mono")
    _check_cpu(R.noise(rate + 3, n, 2, False), rate, "fp32 stereo")
    _check_cpu(torch.from_numpy(R.noise(rate + 4, 5, 2, False)), rate, "a tensor shorter than the filter")


def test_output_lengths():
    for rate, (L, M, _) in SHAPES.items():
        for n in sorted({1, 2, max(M - 1, 1), M, M + 1, 10007}):
            want = -(-n * L // M)
            wavs, lengths = ops.resample_audio([R.noise(n, n, 1, True)], [rate])
            assert lengths.tolist() == [want] and wavs.shape == (1, want), (rate, n)
            assert audioprep.resample_length(n, L, M) == want


def test_ops_resample_audio_batches_pads_and_passes_16_khz_through():
    clips = [R.noise(1, 3000, 2, True), R.noise(2, 999, 1, False), R.noise(3, 1234, 2, False), R.noise(4, 800, 1, True)]
    rates = [44100, 16000, 8000, 16000]
    wavs, lengths = ops.resample_audio(clips, rates)
    assert lengths.tolist() == [1089, 999, 2468, 800] and wavs.shape == (4, 2468)
    for i in (0, 2):
        alone, _ = ops.resample_audio([clips[i]], [rates[i]])
        assert torch.equal(wavs[i, : lengths[i]], alone[0])
    assert torch.equal(wavs[1, :999], torch.from_numpy(clips[1]))                       # untouched, bit for bit
    assert torch.equal(wavs[3, :800], torch.from_numpy(clips[3]).float() / 32768.0)
    for i in range(4):
        assert int((wavs[i, lengths[i]:] != 0).sum()) == 0
    with pytest.raises(ValueError):
        ops.resample_audio(clips, rates[:3])
    with pytest.raises(ValueError, match="positive integer"):
        ops.resample_audio(clips[:1], [44100.0])
    with pytest.raises(ValueError, match="640"):
        ops.resample_audio(clips[:1], [44101])


def test_hub_on_the_cpu_resamples_files_and_pairs(golden_dir, tmp_path):
    hub = _hub(golden_dir)
    pcm = R.noise(21, 30000, 1, True) // 4
    st = R.noise(22, 9000, 2, True) // 4
    fl = R.noise(23, 20000, 1, False)
    path = _write_wav(tmp_path / "a22.wav", pcm, 22050)
    path16 = _write_wav(tmp_path / "b16.wav", st, 16000)
    with pytest.raises(ValueError, match="sample rate: 22050, need 16000"):
        hub.process_audio([path])
    with pytest.raises(ValueError, match="sample rate: 48000, need 16000"):
        hub.process_audio([(fl, 48000)])
    wavs, masks = hub.process_audio([path, (st, 44100), (torch.from_numpy(fl), 48000), path16, (fl, 16000)], resample=True)
    res, res_len = ops.resample_audio([pcm, st, fl], [22050, 44100, 48000])
    assert res_len.tolist() == [R.out_frames(30000, 22050), R.out_frames(9000, 44100), R.out_frames(20000, 48000)]
    want = [audioprep.postprocess(res[i, : res_len[i]]) for i in range(3)] + [audioprep.postprocess(st), audioprep.postprocess(fl)]
    lens = [w.numel() for w in want]
    assert lens == [21769, 16000, 16000, 16000, 20000]  # the 44.1 kHz and 48 kHz clips are under 1 s after resampling: tiled
    assert wavs.shape == (5, max(lens)) and masks.shape == (5, hub._frames(max(lens)) + 1)
    for i, w in enumerate(want):
        assert torch.equal(wavs[i, : lens[i]], w) and int((wavs[i, lens[i]:] != 0).sum()) == 0
        f = hub._frames(lens[i]) + 1
        assert not masks[i, :f].any() and masks[i, f:].all()
    plain, plain_masks = hub.process_audio([path16, fl])                             # 16 kHz items: resample=True changes nothing
    again, again_masks = hub.process_audio([path16, fl], resample=True)
    assert torch.equal(plain, again) and torch.equal(plain_masks, again_masks)
    assert torch.equal(plain[0, :16000], wavs[3, :16000]) and torch.equal(plain[1], wavs[4, :20000])
    direct, direct_len = ops.preprocess_audio([(pcm, 22050)], resample=True)
    assert direct_len.tolist() == [21769] and torch.equal(direct[0], wavs[0, :21769])


def test_the_layer_norm_runs_over_the_whole_resampled_clip_before_the_crop():
    clip = R.noise(31, 48000 * 16, 1, True) // 8  # 16 s at 48 kHz: 256 000 samples at 16 kHz, cropped to 240 000
    clip[700000:] //= 16
    wavs, lengths = ops.preprocess_audio([(clip, 48000)], resample=True)
    res, n = ops.resample_audio([clip], [48000])
    assert n.tolist() == [256000] and lengths.tolist() == [240000]
    assert torch.equal(wavs[0], audioprep.postprocess(res[0]))
    assert not torch.equal(wavs[0], audioprep.postprocess(res[0, :240000]))


def test_device_staging_layout_and_taps():
    """pack_resample: one table per rate, rows of 4 ceil(T / 4) taps = fp32(L h) in the order the kernel reads them, descriptors that
    match include/onepeace_hip.h, and the normaliser's descriptors pointing at the resampled clips behind the host part."""
    clips = [R.noise(41, 5000, 2, True), R.noise(42, 700, 1, False), R.noise(43, 4000, 1, True), R.noise(44, 900, 2, False)]
    rates = [44100, 16000, 44100, 8000]
    p = audioprep.pack_resample(clips, rates, norm=(2000, 1500), pin=False)
    assert p.which == [0, 2, 3] and p.desc.shape == (3, audioprep.RS_DESC_FIELDS) and p.lengths == [1815, 700, 1452, 1800]
    assert p.out_lengths == [1815, 1500, 1500, 1800] and p.T == 1815
    buf = p.host.numpy()
    assert np.array_equal(buf[p.desc_off:p.desc_off + p.desc.nbytes].view(np.int64).reshape(3, -1), p.desc)
    coef = buf[p.coef_off:p.coef_off + 4 * p.coef_count].view(np.float32)
    assert p.coef_off % 16 == 0 and p.coef_count == 160 * 376 + 2 * 140
    for k, i in enumerate(p.which):
        src_off, n, ch, fmt, L, M, T, half, c_off, n_out, dst_off, _ = p.desc[k].tolist()
        a = clips[i]
        assert np.array_equal(buf[src_off:src_off + a.nbytes].view(a.dtype).reshape(a.shape), a) and src_off % 16 == 0
        assert (n, ch, fmt) == (a.shape[0], a.ndim, 0 if a.dtype == np.int16 else 1)
        rl, rm, rhalf, h = R.lowpass(rates[i])
        assert (L, M, half, T) == (rl, rm, rhalf, R.taps(rates[i])) and n_out == p.lengths[i] and dst_off % 16 == 0 and c_off % 4 == 0
        Tp = (T + 3) // 4 * 4
        rows = coef[c_off:c_off + L * Tp].reshape(L, Tp)
        for ph in (0, 1, L // 2, L - 1):
            s = (half - ph) // L
            for t in (0, 1, T // 2, T - 1, Tp - 1):
                idx = ph + (s - t) * L
                want = np.float32(L * h[idx + half]) if abs(idx) <= half and t < T else np.float32(0)
                assert rows[ph, t] == want, (rates[i], ph, t)
        nd = p.norm_desc[i].tolist()
        assert nd[:4] == [p.out_off + dst_off, n_out, 1, 1] and nd[4] == p.out_lengths[i]
    assert p.desc[0, 8] == p.desc[1, 8] and p.desc[0, 10] == 0 and p.desc[1, 10] == 1815 * 4 + 4  # shared table; packed, 16-aligned
    assert p.norm_desc[1].tolist()[:5] == [int(np.ceil(5000 * 4 / 16) * 16), 700, 1, 1, 1500]     # 16 kHz: the staged source itself
    assert p.out_off % 16 == 0 and p.out_off >= buf.size and p.total_bytes == p.out_off + p.out_bytes
    assert np.array_equal(buf[p.norm_desc_off:].view(np.int64).reshape(4, -1), p.norm_desc)
    assert p.norm_desc[:, 5].tolist() == [0, 1, 2, 3] and p.workspace_bytes == 64
    q = audioprep.pack_resample(clips, rates, pin=False)
    assert q.norm_desc is None and q.rows == 1816 and q.desc[:, 10].tolist() == [0, 2 * 1816 * 4, 3 * 1816 * 4] and q.out_bytes == 4 * 1816 * 4
    with pytest.raises(ValueError, match="window"):
        audioprep.pack_resample(clips[:1], [16000 * 40], pin=False)


def test_abi_entry_is_exported_declared_and_bound():
    import importlib.util
    from one_peace_amd import hip
    spec = importlib.util.spec_from_file_location("onepeace_build", os.path.join(ROOT, "one-peace_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib_path = mod.build(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "op_audio_resample" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "onepeace_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+op_audio_resample\s*\(([^;]*?)\)\s*;", header, flags=re.S)
    assert m and len(m.group(1).split(",")) == len(hip.SIGNATURES["op_audio_resample"][1]) == 10
    assert hip.lib().op_abi_version() == 10  # additive
