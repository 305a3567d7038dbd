"""Shared by tests/test_audioresample_cpu.py and tests/test_audioresample_gpu.py: the fp64 oracle of the sample-rate conversion, written
from its definition and from nothing in one-peace_amd:

    L / M = sr_out / sr_in in lowest terms, fc = rolloff min(1, L / M), half = ceil(zeros L / fc),
    h[i] = (fc / L) sinc(i fc / L) kaiser(2 half + 1, beta)[i + half] for i = -half ... half,
    y[n] = L sum_j x[j] h[n M - j L] over 0 <= j < N with |n M - j L| <= half, for n < ceil(N L / M),

and S[n] = L sum_j |x[j] h[n M - j L]|, the scale of the error bound |y - y64| <= (T + 3) 2^-24 S[n], T = floor(2 half / L) + 1: T fused
multiply-adds in any order, one rounding of each coefficient, one for the channel mean and scale, and the final store."""
import math

import numpy as np

RATES = [8000, 11025, 22050, 24000, 32000, 44100, 48000, 88200, 96000]


def lowpass(sr_in, sr_out=16000, zeros=64, rolloff=0.9475, beta=14.769656459379492):
    """(L, M, half, h fp64 [2 half + 1]) from the formula."""
    g = math.gcd(sr_in, sr_out)
    L, M = sr_out // g, sr_in // g
    fc = rolloff * min(1, L / M)
    half = math.ceil(zeros * L / fc)
    i = np.arange(-half, half + 1).astype(np.float64)
    t = i * fc / L
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(np.pi * t) / (np.pi * t))
    return L, M, half, (fc / L) * sinc * np.kaiser(2 * half + 1, beta)


def taps(sr_in, sr_out=16000):
    L, _, half, _ = lowpass(sr_in, sr_out)
    return 2 * half // L + 1


def out_frames(n, sr_in, sr_out=16000):
    g = math.gcd(sr_in, sr_out)
    return -(-n * (sr_out // g) // (sr_in // g))


def mono64(clip):
    """fp64 [N]: int16 PCM as s / 32768, the exact mean over the channels of an [N, C] clip."""
    a = np.asarray(clip)
    x = a.astype(np.float64) / 32768.0 if a.dtype == np.int16 else a.astype(np.float64)
    return x.mean(-1) if x.ndim == 2 else x


def oracle(clip, sr_in, sr_out=16000, rows=None, **kw):
    """(y64, S) at the outputs `rows` (all ceil(N L / M) of them by default)."""
    L, M, half, h = lowpass(sr_in, sr_out, **kw)
    x = mono64(clip)
    N = x.shape[0]
    n_all = np.arange(-(-N * L // M), dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    width = 2 * half // L + 2  # more than the j with |n M - j L| <= half
    y, S = np.empty(n_all.shape[0]), np.empty(n_all.shape[0])
    step = max(1, (1 << 21) // width)
    for c in range(0, n_all.shape[0], step):
        n = n_all[c:c + step, None]
        j = -((half - n * M) // L) + np.arange(width, dtype=np.int64)[None, :]  # from ceil((n M - half) / L) on
        i = n * M - j * L
        ok = (np.abs(i) <= half) & (j >= 0) & (j < N)
        term = np.where(ok, x[np.clip(j, 0, N - 1)] * h[np.clip(i + half, 0, 2 * half)], 0.0)
        y[c:c + step] = L * term.sum(1)
        S[c:c + step] = L * np.abs(term).sum(1)
    return y, S


def bound(S, sr_in, sr_out=16000):
    return (taps(sr_in, sr_out) + 3) * 2.0 ** -24 * S


def worst_ratio(y, y64, limit):
    """The largest |y - y64| / limit (0 where the error is 0, so that a zero limit passes only an exact value)."""
    err = np.abs(np.asarray(y, dtype=np.float64) - y64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(err == 0, 0.0, err / limit).max()) if err.size else 0.0


def noise(seed, n, channels, int16):
    """Full-scale uniform noise: int16 over the whole range, or fp32 in [-1, 1)."""
    g = np.random.default_rng(seed)
    shape = (n,) if channels == 1 else (n, channels)
    if int16:
        return g.integers(-32768, 32768, shape, dtype=np.int64).astype(np.int16)
    return g.uniform(-1.0, 1.0, shape).astype(np.float32)


def constant(n, channels, int16):
    shape = (n,) if channels == 1 else (n, channels)
    return np.full(shape, 23170, dtype=np.int16) if int16 else np.full(shape, 0.70710678, dtype=np.float32)
