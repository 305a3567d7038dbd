"""Host side of the audio pre-processing (one-peace_amd/audioprep.py, ops.preprocess_audio, OnePeaceHubInterface.process_audio) against
tests/golden/audioprep.pt: the outputs of the reference's unmodified BaseDataset.audio_postprocess on seeded clips, its frame counts, and
the reference's own distance from the fp64 oracle (ref_err_over_B).  Needs neither the reference nor a GPU."""
import wave

import numpy as np
import pytest
import torch

from one_peace_amd import audioprep, ops
from tests import audioprep_util as U
from tests.model_util import build_retrieval, load_synth

GATE = 2.5  # x the largest measured ref_err_over_B: the repository's convention for measured gates


@pytest.fixture(scope="module")
def fx(golden_dir):
    return U.load_fixture(golden_dir)


def _hub(golden_dir):
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    mfx = torch.load(golden_dir + "/micro_retrieval.pt", weights_only=False)
    return OnePeaceHubInterface(load_synth(build_retrieval(mfx["cfg"], mfx["vocab"]), mfx["shapes"]), device="cpu", dtype="float32")


def _write_wav(path, pcm, rate=16000, width=2):
    a = np.asarray(pcm)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if a.ndim == 1 else a.shape[1])
        w.setsampwidth(width)
        w.setframerate(rate)
        if width == 2:
            w.writeframes(a.astype("<i2").tobytes())
        elif width == 1:
            w.writeframes(((a.astype(np.int32) >> 8) + 128).astype(np.uint8).tobytes())
        else:
            w.writeframes(b"".join(int(v).to_bytes(3, "little", signed=True) for v in a.reshape(-1).astype(np.int32) << 8))
    return str(path)


def test_fixture_covers_the_cases_and_its_yardstick_is_sane(fx):
    rows = fx["cases"].tolist()
    assert len(rows) >= 12 and {r[1] for r in rows} >= {1, 2, 7, 5000, 15999, 16000, 16001, 28345, 40000, 32001}
    assert {(r[2], r[3]) for r in rows} >= {(1, 0), (2, 0), (1, 1), (2, 1)} and {r[5] for r in rows} == {1, 2}
    assert sum(r[5] == 2 for r in rows) <= 2
    assert 0 < float(fx["ref_err_over_B"].max()) <= 1000


def test_fp64_oracle_is_within_the_reference_s_own_error_of_the_fixture(fx):
    """|fixture - y64| <= 2.5 max(ref_err_over_B) B per element.  A semantic slip in the oracle (unbiased variance, statistics after
    the crop, tiling before normalising) misses this by orders of magnitude on the tiny-n and crop cases."""
    gate = GATE * float(fx["ref_err_over_B"].max())
    for clip, md, want, _ in U.fixture_cases(fx):
        y64, m, r = U.oracle64(U.mono32(clip), U.RATE * md, U.RATE)
        assert y64.shape == want.shape
        ratio = U.worst_ratio(want, y64, U.bound(y64, m, r))
        assert ratio <= gate, (tuple(clip.shape), md, ratio, gate)


def test_oracle_gate_catches_semantic_slips(fx):
    """The gate above is not vacuous: an unbiased variance at n = 7 and statistics taken after the crop both miss it."""
    gate = GATE * float(fx["ref_err_over_B"].max())
    cases = U.fixture_cases(fx)
    clip, md, want, _ = next(c for c in cases if c[0].shape[0] == 7)
    x = U.mono32(clip).double()
    y = ((x - x.mean()) / torch.sqrt(x.var(unbiased=True) + 1e-5)).repeat(16000 // 7 + 1)[:16000]
    _, m, r = U.oracle64(U.mono32(clip), U.RATE * md, U.RATE)
    assert U.worst_ratio(want, y, U.bound(y, m, r)) > 1000 * gate
    clip, md, want, _ = next(c for c in cases if c[0].shape[0] == 40000)
    y, m, r = U.oracle64(U.mono32(clip)[:16000], U.RATE, U.RATE)
    assert U.worst_ratio(want, y, U.bound(y, m, r)) > 100 * gate


def test_postprocess_meets_the_gate_and_the_fixture_s_structure(fx):
    gate = GATE * float(fx["ref_err_over_B"].max())
    for clip, md, want, _ in U.fixture_cases(fx):
        for src in (clip, clip.numpy()):
            got = audioprep.postprocess(src, U.RATE, max_seconds=md)
            assert got.dtype == torch.float32 and got.shape == want.shape
        y64, m, r = U.oracle64(U.mono32(clip), U.RATE * md, U.RATE)
        ratio = U.worst_ratio(got, y64, U.bound(y64, m, r))
        assert ratio <= gate, (tuple(clip.shape), md, ratio, gate)
        n = min(clip.shape[0], U.RATE * md)
        if n < U.RATE:  # tiled: period n, bit for bit, in the reference's output and here
            idx = torch.arange(U.RATE) % n
            assert torch.equal(want, want[:n][idx]) and torch.equal(got, got[:n][idx])
        assert audioprep.out_length(clip.shape[0], U.RATE * md, U.RATE) == want.numel()


def test_preprocess_audio_cpu_pads_with_zeros_and_reports_lengths(fx):
    for md in (1, 2):
        cases = [c for c in U.fixture_cases(fx) if c[1] == md]
        wavs, lengths = ops.preprocess_audio([c[0] for c in cases], U.RATE, max_seconds=md)
        assert wavs.dtype == torch.float32 and lengths.dtype == torch.int64
        assert lengths.tolist() == [c[2].numel() for c in cases] and wavs.shape == (len(cases), max(lengths.tolist()))
        for i, (clip, _, want, _) in enumerate(cases):
            L = want.numel()
            assert torch.equal(wavs[i, :L], audioprep.postprocess(clip, U.RATE, max_seconds=md))
            assert int((wavs[i, L:] != 0).sum()) == 0
    bf, _ = ops.preprocess_audio([c[0] for c in cases], U.RATE, max_seconds=2, dtype=torch.bfloat16)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, wavs.to(torch.bfloat16))


def test_hub_masks_equal_the_reference_frame_counts(golden_dir, fx):
    hub = _hub(golden_dir)
    cases = [c for c in U.fixture_cases(fx) if c[1] == 1]  # the hub crops at 15 s; these clips are shorter than that
    long = U.source_clip(77, 16000 * 15 + 3, 1, U.FMT_S16, U.NOISE, 0.0, 0.3)
    wavs, masks = hub.process_audio([c[0] for c in cases] + [long])
    lens = [max(min(c[0].shape[0], 240000), 16000) for c in cases] + [240000]
    assert wavs.shape == (len(lens), 240000) and masks.dtype == torch.bool
    by_len = {c[2].numel(): c[3] for c in U.fixture_cases(fx)}  # the reference's frames per output length
    assert hub._frames(16000) == by_len[16000] and hub._frames(28345) == by_len[28345] and hub._frames(32000) == by_len[32000]
    for i, L in enumerate(lens):
        f = hub._frames(L) + 1
        assert not masks[i, :f].any() and masks[i, f:].all()
        assert int((wavs[i, L:] != 0).sum()) == 0


def test_read_wav_round_trip_and_refusals(tmp_path):
    g = torch.Generator().manual_seed(3)
    mono = torch.randint(-32768, 32768, (1234,), generator=g).to(torch.int16).numpy()
    stereo = torch.randint(-32768, 32768, (999, 2), generator=g).to(torch.int16).numpy()
    a, rate = audioprep.read_wav(_write_wav(tmp_path / "m.wav", mono))
    assert rate == 16000 and a.dtype == np.int16 and a.shape == (1234,) and np.array_equal(a, mono)
    a, rate = audioprep.read_wav(_write_wav(tmp_path / "s.wav", stereo, rate=44100))
    assert rate == 44100 and a.dtype == np.int16 and a.shape == (999, 2) and np.array_equal(a, stereo)
    with pytest.raises(ValueError, match="sample rate: 44100, need 16000"):
        audioprep.as_clip(str(tmp_path / "s.wav"))
    with pytest.raises(ValueError, match="8-bit"):
        audioprep.read_wav(_write_wav(tmp_path / "w8.wav", mono, width=1))
    with pytest.raises(ValueError, match="24-bit"):
        audioprep.read_wav(_write_wav(tmp_path / "w24.wav", mono, width=3))
    assert np.array_equal(audioprep.as_clip(tmp_path / "m.wav"), mono)  # a PathLike works too


def test_as_clip_inputs_and_refusals():
    g = torch.Generator().manual_seed(4)
    f = torch.randn(100, generator=g)
    assert audioprep.as_clip(f).dtype == np.float32 and np.array_equal(audioprep.as_clip(f.double().numpy()), f.numpy())
    assert audioprep.as_clip(f[:, None]).shape == (100,)
    multi = torch.randn(50, 5, generator=g)
    assert np.array_equal(audioprep.as_clip(multi), multi.mean(-1).numpy())  # C > 2: feats.mean(-1) on the host
    pcm = torch.randint(-32768, 32768, (64, 2), generator=g).to(torch.int16)
    assert audioprep.as_clip(pcm).dtype == np.int16 and audioprep.as_clip(pcm).shape == (64, 2)
    for bad in (torch.zeros(0), np.zeros((0, 2), dtype=np.int16), torch.zeros(2, 3, 4), torch.zeros(()), torch.zeros(5, dtype=torch.int32)):
        with pytest.raises(ValueError):
            audioprep.as_clip(bad)
    with pytest.raises(ValueError):
        ops.preprocess_audio([torch.zeros(0)])


def test_pack_clips_layout():
    g = torch.Generator().manual_seed(5)
    clips = [torch.randint(-100, 100, (7,), generator=g).to(torch.int16), torch.randn(20001, 2, generator=g),
             torch.randint(-100, 100, (8193, 2), generator=g).to(torch.int16), torch.randn(3, generator=g)]
    p = audioprep.pack_clips(clips, max_len=20000, min_len=10, pin=False)
    assert len(p) == 4 and p.desc.shape == (4, audioprep.DESC_FIELDS) and p.desc.dtype == np.int64
    assert p.lengths == [10, 20000, 8193, 10] and p.T == 20000 and (p.max_len, p.min_len) == (20000, 10)
    buf = p.host.numpy()
    off, part = 0, 0
    for i, c in enumerate(clips):
        a = c.numpy()
        src_off, n, ch, fmt, L, part_off = p.desc[i].tolist()
        assert src_off == off and src_off % 16 == 0 and (n, ch) == (a.shape[0], a.ndim) and L == p.lengths[i] and part_off == part
        assert fmt == (audioprep.FMT_S16 if a.dtype == np.int16 else audioprep.FMT_F32)
        assert np.array_equal(buf[src_off:src_off + a.nbytes].view(a.dtype).reshape(a.shape), a)
        off = (off + a.nbytes + 15) // 16 * 16
        part += -(-n // audioprep.STAT_CHUNK)
    assert p.src_bytes == off == p.desc_off and p.desc_off % 16 == 0 and p.workspace_bytes == part * 16
    assert np.array_equal(buf[p.desc_off:].view(np.int64).reshape(4, -1), p.desc) and buf.size == p.desc_off + p.desc.nbytes
    with pytest.raises(ValueError):
        audioprep.pack_clips(clips, max_len=10, min_len=20, pin=False)


def test_hub_on_the_cpu_with_paths_int16_and_float_inputs_mixed(golden_dir, tmp_path):
    hub = _hub(golden_dir)
    pcm = U.source_clip(11, 30000, 1, U.FMT_S16, U.TRIANGLE, 0.0, 0.4)
    st = U.source_clip(12, 5000, 2, U.FMT_S16, U.NOISE, 0.1, 0.2)
    fl = U.source_clip(13, 20000, 1, U.FMT_F32, U.NOISE, 0.0, 0.5)
    paths = [_write_wav(tmp_path / "a.wav", pcm.numpy()), _write_wav(tmp_path / "b.wav", st.numpy())]
    wavs, masks = hub.process_audio([paths[0], st.numpy(), fl, paths[1], pcm.float() / 32768])
    want = [audioprep.postprocess(c) for c in (pcm, st, fl, st, pcm)]
    assert wavs.shape == (5, 30000) and masks.shape == (5, hub._frames(30000) + 1)
    for i, w in enumerate(want):
        assert torch.equal(wavs[i, : w.numel()], w) and int((wavs[i, w.numel():] != 0).sum()) == 0
        assert int((~masks[i]).sum()) == hub._frames(w.numel()) + 1
    assert torch.equal(wavs[0], wavs[4]) and torch.equal(wavs[1], wavs[3])  # a file = its PCM = its samples / 32768
    old = torch.nn.functional.layer_norm(fl, fl.shape)  # what process_audio computed for a 1-D float waveform before
    assert torch.equal(wavs[2, :20000], old)
    _write_wav(tmp_path / "c.wav", pcm.numpy(), rate=22050)
    with pytest.raises(ValueError, match="sample rate: 22050, need 16000"):
        hub.process_audio([str(tmp_path / "c.wav")])
    with pytest.raises(ValueError):
        hub.process_audio([torch.zeros(0)])
    with pytest.raises(ValueError):
        hub.process_audio([torch.zeros(2, 3, 4)])
