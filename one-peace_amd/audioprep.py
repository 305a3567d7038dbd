"""Host side of the audio pre-processing of the hub (one_peace/models/one_peace/hub_interface.py:170-193) and the datasets
(data/base_dataset.py:53-102, ``read_audio`` + ``audio_postprocess``): decode, mean over the channels, ``F.layer_norm`` over the
whole clip, crop to ``max_len`` samples, repeat the normalised clip up to ``min_len``, right-pad with zeros.

``read_wav`` decodes 16-bit PCM WAV files with the standard library; ``as_clip`` takes whatever a caller may hand over (a path,
int16 PCM, float samples) to the two sample formats the device kernel reads; ``pack_clips`` stages a batch and its descriptor
table for one host-to-device copy (csrc/audioprep.hip, op_audio_normalize_pad); ``postprocess`` is the same arithmetic in torch:
the CPU route of ops.preprocess_audio and the CPU reference of the tests.  Resampling is not provided: the reference's datasets
refuse any rate but 16 kHz (base_dataset.py:88-89) and so does this module."""
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
