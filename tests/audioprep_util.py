"""Shared by tests/test_audioprep_cpu.py and tests/test_audioprep_gpu.py: the seeded sources, the fp64 oracle and the bound of
tests/golden/make_audioprep_golden.py (the same function bodies), and the fixture's cases."""
import os

import torch

RATE = 16000
FMT_S16, FMT_F32 = 0, 1
NOISE, TRIANGLE, CONSTANT, FULL_SCALE = 0, 1, 2, 3


def source_clip(seed, n, channels, fmt, kind, dc, amp):  # = make_audioprep_golden.py: source_clip
    g = torch.Generator().manual_seed(seed)
    u = torch.rand((n, channels), generator=g, dtype=torch.float64)
    if kind == NOISE:
        x = dc + amp * (2 * u - 1)
    elif kind == TRIANGLE:
        period = 37 + seed % 64
        t = (torch.arange(n, dtype=torch.int64)[:, None] + 5 * torch.arange(channels, dtype=torch.int64)[None, :]) % period
        x = dc + amp * ((2 * t - period).abs().double() / period * 2 - 1)
    elif kind == CONSTANT:
        x = torch.full((n, channels), dc, dtype=torch.float64)
    else:
        x = dc + amp * torch.where(u < 0.5, -1.0, 1.0).double()
    if fmt == FMT_S16:
        x = torch.clamp(torch.round(x * 32768), -32768, 32767).to(torch.int16)
    else:
        x = x.to(torch.float32)
    return x[:, 0].contiguous() if channels == 1 else x.contiguous()


def mono32(clip):  # = make_audioprep_golden.py: mono32
    x = clip.to(torch.float32) / 32768.0 if clip.dtype == torch.int16 else clip
    return x.mean(-1) if x.dim() == 2 else x


def oracle64(x32, max_len, min_len):  # = make_audioprep_golden.py: oracle64
    x = x32.double()
    m = x.mean()
    r = 1.0 / torch.sqrt(((x - m) ** 2).mean() + 1e-5)
    y = ((x - m) * r)[:max_len]
    if y.numel() < min_len:
        y = y.repeat(-(-min_len // y.numel()))[:min_len]
    return y, float(m), float(r)


def bound(y64, m, r):
    """B = 2^-24 (4 |y64| + 2 |m| r): one rounding each for m, r, the difference and the product, plus the cancellation term."""
    return 2.0 ** -24 * (4 * y64.abs() + 2 * abs(m) * r)


def bound_bf16(y64, m, r):
    B = bound(y64, m, r)
    return 2.0 ** -8 * (y64.abs() + B) + B


def worst_ratio(y, y64, limit):
    """The largest |y - y64| / limit over the elements (0 where the error is 0, so that a zero limit passes only an exact value)."""
    err = (y.double() - y64).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / limit).max())


def load_fixture(golden_dir):
    return torch.load(os.path.join(golden_dir, "audioprep.pt"), weights_only=False)


def fixture_cases(fx):
    """[(clip, max_duration, reference output, reference frame count)] of the fixture."""
    out = []
    for (seed, n, ch, fmt, kind, md), (dc, amp), want, frames in zip(fx["cases"].tolist(), fx["dc_amp"].tolist(), fx["outputs"],
                                                                     fx["frames"].tolist()):
        out.append((source_clip(seed, n, ch, fmt, kind, dc, amp), md, want, frames))
    return out


# the case list in full: every source kind x every length, at max_duration 1 and 2 (the fixture holds a dozen of them)
LENGTHS = [1, 2, 7, 5000, 15999, 16000, 16001, 28345]
SOURCES = [(1, FMT_S16), (2, FMT_S16), (1, FMT_F32), (2, FMT_F32)]
SIGNALS = [(NOISE, 0.0, 0.3), (TRIANGLE, 0.1, 0.5), (NOISE, 0.5, 1e-3), (CONSTANT, 0.25, 0.0), (FULL_SCALE, 0.0, 1.0)]


def cross_product(max_duration):
    """Seeded clips over SOURCES x (LENGTHS, max_len + 1, 2.5 max_len) x SIGNALS."""
    max_len = RATE * max_duration
    clips, seed = [], 5000 + max_duration
    for n in LENGTHS + [max_len + 1, max_len * 5 // 2]:
        for ch, fmt in SOURCES:
            for kind, dc, amp in SIGNALS:
                seed += 1
                clips.append(source_clip(seed, n, ch, fmt, kind, dc, amp))
    return clips
