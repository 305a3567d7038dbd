"""Host side of the audio pre-processing of the hub (one_peace/models/one_peace/hub_interface.py:170-193) and the datasets
(data/base_dataset.py:53-102, ``read_audio`` + ``audio_postprocess``): decode, mean over the channels, ``F.layer_norm`` over the
whole clip, crop to ``max_len`` samples, repeat the normalised clip up to ``min_len``, right-pad with zeros.

``read_wav`` decodes 16-bit PCM WAV files with the standard library; ``as_clip`` takes whatever a caller may hand over (a path,
int16 PCM, float samples) to the two sample formats the device kernel reads; ``pack_clips`` stages a batch and its descriptor
table for one host-to-device copy (csrc/audioprep.hip, op_audio_normalize_pad); ``postprocess`` is the same arithmetic in torch:
the CPU route of ops.preprocess_audio and the CPU reference of the tests.

The reference's datasets refuse any rate but 16 kHz (base_dataset.py:88-89) and so do ``check_rate`` / ``as_clip``; its hub resamples
with librosa.load(sr=16000), i.e. soxr (hub_interface.py:170-175).  ``resample_filter`` defines this project's own low-pass in closed
form (a Kaiser-windowed sinc, polyphase L / M), ``resample`` applies it on the host in fp64 and ``pack_resample`` stages a batch, its
descriptors and the fp32 coefficient tables for the device kernel (csrc/audioresample.hip, op_audio_resample).  Features of resampled
audio differ from the reference's by the difference between the two low-pass filters; clips already at the target rate are untouched."""
import functools
import math
import os
import wave

import numpy as np
import torch
import torch.nn.functional as F

FMT_S16, FMT_F32 = 0, 1   # sample formats of op_audio_normalize_pad
STAT_CHUNK = 8192         # frames per statistics partial (csrc/audioprep.hip: AP_CHUNK)
PARTIAL_BYTES = 16
MAX_FRAMES = 1 << 27
DESC_FIELDS = 6           # int64 per clip: src_off, frames, channels, format, out_len, part_off (include/onepeace_hip.h)
MAX_PHASES = 640          # largest L of a resampling ratio L / M (csrc/audioresample.hip: AR_MAX_L)
RS_DESC_FIELDS = 12       # int64 per resampled clip: src_off, frames, channels, format, L, M, T, half, coef_off, out_frames, dst_off, 0
RS_OUT, RS_WINDOW = 256, 8192  # outputs per workgroup and fp32 samples of its staged input window (AR_OUT, AR_WINDOW)


def read_wav(path):
    """(int16 [n] or [n, 2], sample_rate) of a 16-bit PCM WAV file, through the standard library's ``wave``.  Other sample widths,
    more than two channels and compressed files are a ValueError that names what was found.  A file ``wave`` cannot read goes to
    ``soundfile`` where that is installed (FLAC, float WAV ...); nothing here requires it."""
    try:
        with wave.open(os.fspath(path), "rb") as w:
            ch, width, rate, n, comp = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes(), w.getcomptype()
            if comp != "NONE":
                raise ValueError("%s: compression %r, need uncompressed 16-bit PCM" % (path, comp))
            if width != 2:
                raise ValueError("%s: %d-bit samples, need 16-bit PCM" % (path, 8 * width))
            if ch not in (1, 2):
                raise ValueError("%s: %d channels, need 1 or 2" % (path, ch))
            data = w.readframes(n)
    except wave.Error as e:
        try:
            import soundfile
        except ImportError:
            raise ValueError("%s: not a PCM WAV file the wave module reads (%s)" % (path, e)) from None
        a, rate = soundfile.read(os.fspath(path), dtype="float32")  # base_dataset.py:53-55
        return a, int(rate)
    a = np.frombuffer(data, dtype="<i2").astype(np.int16)
    a = a[: len(a) // ch * ch]
    return (a.reshape(-1, 2) if ch == 2 else a), int(rate)


def check_rate(rate, sample_rate=16000):
    """base_dataset.py:88-89: a clip at another rate is refused, not resampled."""
    if int(rate) != int(sample_rate):
        raise ValueError("sample rate: %d, need %d" % (rate, sample_rate))


def as_clip(item, sample_rate=16000):
    """The contiguous numpy clip of one input: int16 [n] or [n, 2] (PCM; value s / 32768), or float32 [n] or [n, 2].  Accepted:
    int16 [n] / [n, 2], float [n] / [n, C] arrays or tensors (C > 2 is averaged here in fp32, as feats.mean(-1); C = 1 is
    squeezed), or the path of a WAV file at `sample_rate`.  An empty clip is refused: the reference divides by zero on it."""
    if isinstance(item, (str, bytes, os.PathLike)):
        a, rate = read_wav(item)
        check_rate(rate, sample_rate)
    else:
        a = item.detach().cpu().numpy() if torch.is_tensor(item) else np.asarray(item)
    if a.ndim not in (1, 2):
        raise ValueError("an audio clip must be [n] or [n, channels], got shape %s" % (tuple(a.shape),))
    if a.shape[0] < 1 or (a.ndim == 2 and a.shape[1] < 1):
        raise ValueError("an audio clip must hold at least one sample, got shape %s" % (tuple(a.shape),))
    if a.shape[0] > MAX_FRAMES:
        raise ValueError("an audio clip may hold up to 2^27 frames, got %d" % a.shape[0])
    if a.dtype != np.int16 and a.dtype.kind != "f":
        raise ValueError("an audio clip must be int16 PCM or floating point, got %s" % a.dtype)
    if a.ndim == 2 and a.shape[1] == 1:
        a = a[:, 0]
    if a.ndim == 2 and a.shape[1] > 2:
        a = a.astype(np.float32) / 32768.0 if a.dtype == np.int16 else a
        a = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).mean(-1).numpy()
    return np.ascontiguousarray(a if a.dtype == np.int16 else a.astype(np.float32, copy=False))


def out_length(n, max_len, min_len):
    """Samples of a clip of n frames after the crop to max_len and the tiling up to min_len."""
    return max(min(n, max_len), min_len)


def postprocess(clip, sample_rate=16000, max_seconds=15, min_seconds=1):
    """fp32 [out_length]: base_dataset.py:84-102 (= hub_interface.py:176-186 for max_seconds 15) of one decoded clip, in torch on the
    host: mean over the channels, F.layer_norm over the whole clip, crop to sample_rate * max_seconds samples from the start, and a
    clip shorter than sample_rate * min_seconds repeated up to that length.  int16 PCM is taken as s / 32768."""
    w = torch.as_tensor(clip)
    w = w.to(torch.float32) / 32768.0 if w.dtype == torch.int16 else w.to(torch.float32)
    if w.dim() == 2:
        w = w.mean(-1)
    w = F.layer_norm(w, w.shape)
    max_len, min_len = int(sample_rate * max_seconds), int(sample_rate * min_seconds)
    if w.numel() > max_len:
        w = w[:max_len]
    if w.numel() < min_len:
        w = w.repeat(math.ceil(min_len / w.numel()))[:min_len]
    return w


class PackedClips:
    """A batch of decoded clips staged for op_audio_normalize_pad.

    Layout of the ONE buffer (pinned on the host, copied to the device with one H2D copy): the clips back to back, each at a
    16-byte aligned offset (`src_bytes` in all), then the descriptor table int64 [B, DESC_FIELDS] at `desc_off`.  `desc` is the
    host copy of the table; `lengths` the output samples per clip, `T` their maximum (the width of the batch) and
    `workspace_bytes` the size of the statistics partials (16 bytes per STAT_CHUNK frames of each clip)."""

    def __init__(self, host, desc, src_bytes, desc_off, workspace_bytes, lengths, max_len, min_len):
        self.host, self.desc, self.src_bytes, self.desc_off, self.workspace_bytes = host, desc, src_bytes, desc_off, workspace_bytes
        self.lengths, self.max_len, self.min_len = lengths, max_len, min_len
        self.T = max(lengths) if lengths else 0

    def __len__(self):
        return self.desc.shape[0]


def _align(n, a=16):
    return (n + a - 1) // a * a


def pack_clips(clips, max_len, min_len, pin=True):
    """PackedClips of as_clip() arrays (int16 or float32, [n] or [n, 2]) for a crop to max_len and tiling up to min_len samples."""
    max_len, min_len = int(max_len), int(min_len)
    if not (0 <= min_len <= max_len and 1 <= max_len <= MAX_FRAMES):
        raise ValueError("pack_clips: need 0 <= min_len <= max_len and 1 <= max_len <= 2^27, got %d / %d" % (min_len, max_len))
    arrs = [as_clip(c) for c in clips]
    B = len(arrs)
    desc = np.zeros((B, DESC_FIELDS), dtype=np.int64)
    src_off, part_off, lengths = 0, 0, []
    for i, a in enumerate(arrs):
        n, ch = a.shape[0], (a.shape[1] if a.ndim == 2 else 1)
        lengths.append(out_length(n, max_len, min_len))
        desc[i] = (src_off, n, ch, FMT_S16 if a.dtype == np.int16 else FMT_F32, lengths[-1], part_off)
        src_off = _align(src_off + a.nbytes)
        part_off += (n + STAT_CHUNK - 1) // STAT_CHUNK
    src_bytes = desc_off = max(src_off, 16)
    host = torch.empty(desc_off + desc.nbytes, dtype=torch.uint8, pin_memory=pin)
    buf = host.numpy()
    for i, a in enumerate(arrs):
        o = int(desc[i, 0])
        buf[o:o + a.nbytes] = a.reshape(-1).view(np.uint8)
        buf[o + a.nbytes:_align(o + a.nbytes)] = 0
    buf[desc_off:] = desc.view(np.uint8).reshape(-1)
    return PackedClips(host, desc, src_bytes, desc_off, part_off * PARTIAL_BYTES, lengths, max_len, min_len)


# ---- sample-rate conversion: a polyphase Kaiser-windowed sinc, defined here (csrc/audioresample.hip applies it on the device) --------
def _check_rates(sr_in, sr_out):
    for what, r in (("input", sr_in), ("output", sr_out)):
        if isinstance(r, bool) or not isinstance(r, (int, np.integer)) or r < 1:
            raise ValueError("resampling: the %s sample rate must be a positive integer, got %r" % (what, r))


def resample_filter(sr_in, sr_out=16000, zeros=64, rolloff=0.9475, beta=14.769656459379492):
    """(L, M, h): the ratio sr_out / sr_in = L / M in lowest terms and the fp64 low-pass h[-half ... half] (stored at h[i + half]) at the
    rate L * sr_in: h[i] = (fc / L) sinc(i fc / L) kaiser(2 half + 1, beta)[i + half] with fc = rolloff * min(1, L / M) (the cut-off as
    a fraction of the lower Nyquist frequency) and half = ceil(zeros * L / fc) (`zeros` zero crossings of the sinc on each side).  The
    resampled clip is y[n] = L sum_j x[j] h[n M - j L]: scipy.signal.resample_poly(x, L, M, window=h).  Rates must be positive integers
    and L at most MAX_PHASES (8000, 11025, 22050, 24000, 32000, 44100, 48000, 88200 and 96000 Hz to 16000 Hz all fit)."""
    _check_rates(sr_in, sr_out)
    g = math.gcd(int(sr_in), int(sr_out))
    L, M = int(sr_out) // g, int(sr_in) // g
    if L > MAX_PHASES:
        raise ValueError("resampling %d Hz to %d Hz needs L = %d filter phases, at most %d are supported" % (sr_in, sr_out, L, MAX_PHASES))
    fc = rolloff * min(1, L / M)
    half = math.ceil(zeros * L / fc)
    i = np.arange(-half, half + 1, dtype=np.float64)
    return L, M, (fc / L) * np.sinc(i * fc / L) * np.kaiser(2 * half + 1, beta)


def resample_length(n, L, M):
    """Samples of a clip of n frames after resampling by L / M: ceil(n L / M)."""
    return -(-int(n) * L // M)


def resample_rows(L, h, pad=1, scale=1.0):
    """(T, rows fp64 [L, Tp]): the polyphase form of h.  Output n has the phase p = n M mod L and reads the inputs j = q - s + t,
    t = 0 ... T - 1, with q = floor(n M / L), s = floor((half - p) / L) and T = floor(2 half / L) + 1; rows[p, t] = scale * h[p + (s - t) L],
    0 where that index is outside the filter and for T <= t < Tp = T rounded up to a multiple of `pad`."""
    half = (h.shape[0] - 1) // 2
    T = 2 * half // L + 1
    Tp = -(-T // pad) * pad
    p = np.arange(L, dtype=np.int64)[:, None]
    idx = p + ((half - p) // L - np.arange(Tp, dtype=np.int64)[None, :]) * L
    ok = (np.abs(idx) <= half) & (np.arange(Tp)[None, :] < T)
    return T, np.where(ok, scale * h[np.clip(idx + half, 0, 2 * half)], 0.0)


@functools.lru_cache(maxsize=16)
def _device_table(sr_in, sr_out):
    """(L, M, T, half, fp32 [L, Tp]) of the default filter: the device kernel's taps fp32(L h), each row padded to 16 bytes."""
    L, M, h = resample_filter(sr_in, sr_out)
    T, rows = resample_rows(L, h, pad=4, scale=float(L))
    return L, M, T, (h.shape[0] - 1) // 2, np.ascontiguousarray(rows, dtype=np.float32)


def mono64(clip):
    """fp64 [n] of an as_clip() array: s / 32768 for int16 PCM, the exact mean over two channels."""
    x = clip.astype(np.float64) / 32768.0 if clip.dtype == np.int16 else clip.astype(np.float64)
    return x.mean(-1) if x.ndim == 2 else x


def resample(clip, sr_in, sr_out=16000, **filter_kw):
    """fp32 [ceil(n L / M)] of an as_clip() array on the host: y[n] = L sum_j x[j] h[n M - j L] over the samples of the clip (zero
    outside it), x the fp64 mono signal, accumulated in fp64 and rounded once to fp32.  A clip at sr_out needs no filter: use it as
    it is."""
    L, M, h = resample_filter(sr_in, sr_out, **filter_kw)
    T, rows = resample_rows(L, h)
    half = (h.shape[0] - 1) // 2
    x = mono64(clip)
    n_out, K = resample_length(x.shape[0], L, M), half // L
    xp = np.concatenate([np.zeros(K + 1), x, np.zeros(T + 1)])  # input j at xp[j + K + 1]; every index below stays inside
    y = np.empty(n_out, dtype=np.float64)
    step = max(1, (1 << 22) // T)
    for n0 in range(min(L, n_out)):  # the outputs n0, n0 + L, ... share the phase p; their first inputs are M apart
        p = n0 * M % L
        first = n0 * M // L - (half - p) // L + K + 1
        cnt = (n_out - n0 + L - 1) // L
        for c0 in range(0, cnt, step):
            c1 = min(cnt, c0 + step)
            win = np.lib.stride_tricks.as_strided(xp[first + c0 * M:], shape=(c1 - c0, T), strides=(M * xp.strides[0], xp.strides[0]),
                                                  writeable=False)
            y[n0 + c0 * L:n0 + c1 * L:L] = L * np.einsum("ct,t->c", win, rows[p])  # (no copy of the overlapping windows)
    return y.astype(np.float32)


class PackedResample:
    """A batch staged for op_audio_resample, optionally followed by op_audio_normalize_pad on the device.

    Layout of the ONE host buffer (copied to the start of a device buffer of `total_bytes` with one H2D copy): every clip back to back
    at 16-byte aligned offsets (`src_bytes`), the resampler's descriptor table int64 [R, RS_DESC_FIELDS] at `desc_off` (one row per
    clip of `which`, the clips at another rate), the coefficient tables fp32 [`coef_count`] at `coef_off` (one table per distinct
    rate, each row 16-byte aligned) and, with `norm`, the normaliser's table int64 [B, DESC_FIELDS] at `norm_desc_off`.  The kernel's
    outputs are mono fp32 clips at `out_off` + their `dst_off`: behind the host part in the same device buffer (the normaliser's
    descriptors point there, and at the staged source for clips already at the target rate), or rows of a [B, row] matrix of its own
    (`rows` = the row length) for ops.resample_audio.  `lengths`: resampled frames per clip of the batch."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def __len__(self):
        return len(self.lengths)


def pack_resample(clips, rates, sample_rate=16000, norm=None, pin=True):
    """PackedResample of as_clip() arrays at `rates`.  norm = (max_len, min_len): also the descriptor table of a following
    op_audio_normalize_pad over the resampled (or, at `sample_rate`, the staged) clips; norm = None: the outputs are rows of a
    [B, rows] fp32 matrix, `rows` = the longest resampled clip rounded up to 4 samples."""
    arrs = [as_clip(c) for c in clips]
    B = len(arrs)
    if len(rates) != B:
        raise ValueError("pack_resample: %d clips and %d rates" % (B, len(rates)))
    for i in range(B):
        _check_rates(rates[i], sample_rate)
    which = [i for i in range(B) if int(rates[i]) != int(sample_rate)]
    tables, coef_count = {}, 0
    for i in which:
        r = int(rates[i])
        if r not in tables:
            L, M, T, half, rows = _device_table(r, int(sample_rate))
            if (RS_OUT - 1) * M // L + rows.shape[1] + 2 > RS_WINDOW:
                raise ValueError("resampling %d Hz to %d Hz on the device: a window of %d samples per %d outputs, at most %d are supported"
                                 % (r, sample_rate, (RS_OUT - 1) * M // L + rows.shape[1] + 2, RS_OUT, RS_WINDOW))
            tables[r] = (L, M, T, half, rows, coef_count)
            coef_count += rows.size
    lengths, src_offs, src_off = [], [], 0
    for i, a in enumerate(arrs):
        src_offs.append(src_off)
        src_off = _align(src_off + a.nbytes)
        if int(rates[i]) != int(sample_rate):
            L, M = tables[int(rates[i])][:2]
            lengths.append(resample_length(a.shape[0], L, M))
            if lengths[-1] > MAX_FRAMES:
                raise ValueError("a resampled audio clip may hold up to 2^27 frames, got %d" % lengths[-1])
        else:
            lengths.append(a.shape[0])
    src_bytes = desc_off = max(src_off, 16)
    rs_desc = np.zeros((len(which), RS_DESC_FIELDS), dtype=np.int64)
    coef_off = _align(desc_off + rs_desc.nbytes)
    norm_desc_off = _align(coef_off + 4 * coef_count)
    host_bytes = norm_desc_off + (B * DESC_FIELDS * 8 if norm is not None else 0)
    rows = _align(max(lengths, default=0), 4)
    out_off, dst = _align(host_bytes), 0
    for k, i in enumerate(which):
        a = arrs[i]
        L, M, T, half, _, c_off = tables[int(rates[i])]
        dst_off = dst if norm is not None else i * rows * 4
        rs_desc[k] = (src_offs[i], a.shape[0], a.shape[1] if a.ndim == 2 else 1, FMT_S16 if a.dtype == np.int16 else FMT_F32, L, M, T, half,
                      c_off, lengths[i], dst_off, 0)
        dst = _align(dst + 4 * lengths[i])
    out_bytes = max(dst, 16) if norm is not None else max(B * rows * 4, 16)
    norm_desc, out_lengths, part_off = None, None, 0
    if norm is not None:
        max_len, min_len = int(norm[0]), int(norm[1])
        if not (0 <= min_len <= max_len and 1 <= max_len <= MAX_FRAMES):
            raise ValueError("pack_resample: need 0 <= min_len <= max_len and 1 <= max_len <= 2^27, got %d / %d" % (min_len, max_len))
        norm_desc, out_lengths = np.zeros((B, DESC_FIELDS), dtype=np.int64), []
        dst_of = {i: int(rs_desc[k, 10]) for k, i in enumerate(which)}
        for i, a in enumerate(arrs):
            out_lengths.append(out_length(lengths[i], max_len, min_len))
            if i in dst_of:
                norm_desc[i] = (out_off + dst_of[i], lengths[i], 1, FMT_F32, out_lengths[-1], part_off)
            else:
                norm_desc[i] = (src_offs[i], a.shape[0], a.shape[1] if a.ndim == 2 else 1, FMT_S16 if a.dtype == np.int16 else FMT_F32,
                                out_lengths[-1], part_off)
            part_off += (lengths[i] + STAT_CHUNK - 1) // STAT_CHUNK
    host = torch.zeros(host_bytes, dtype=torch.uint8, pin_memory=pin)
    buf = host.numpy()
    for i, a in enumerate(arrs):
        buf[src_offs[i]:src_offs[i] + a.nbytes] = a.reshape(-1).view(np.uint8)
    buf[desc_off:desc_off + rs_desc.nbytes] = rs_desc.view(np.uint8).reshape(-1)
    for L, M, T, half, tab, c_off in tables.values():
        buf[coef_off + 4 * c_off:coef_off + 4 * (c_off + tab.size)] = tab.reshape(-1).view(np.uint8)
    if norm is not None:
        buf[norm_desc_off:] = norm_desc.view(np.uint8).reshape(-1)
    return PackedResample(host=host, src_bytes=src_bytes, desc=rs_desc, desc_off=desc_off, coef_off=coef_off, coef_count=coef_count,
                          norm_desc=norm_desc, norm_desc_off=norm_desc_off, out_off=out_off if norm is not None else 0,
                          out_bytes=out_bytes, total_bytes=out_off + out_bytes if norm is not None else host_bytes, which=which,
                          lengths=lengths, rows=rows, out_lengths=out_lengths, workspace_bytes=part_off * PARTIAL_BYTES,
                          max_len=None if norm is None else int(norm[0]), min_len=None if norm is None else int(norm[1]),
                          T=max(out_lengths) if out_lengths else 0)
