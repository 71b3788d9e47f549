"""numpy statements of Fourier Domain Adaptation (Yang & Soatto, CVPR 2020) for the tests of
csrc/fda.hip, and the inputs those tests share.  No torch.

``fda_fft`` is the published formulation in fp64 (the oracle).  ``band_spectrum`` / ``apply_band``
restate the kernels' formulas, which touch only the band |u|, |v| <= b:

    out(y,x) = src(y,x) + 1/(hw) * sum_{(u,v) in band} D(u,v) e^{2 pi i (uy/h + vx/w)}
    D = strength * (A_t - A_s) * F_s / A_s         A_s = |F_s|; D = strength * A_t where A_s == 0

in fp64 (equal to the oracle up to rounding) or in fp32 (what the number format costs: the GPU
tolerances are multiples of this restatement's own error, tests/pinned/fda_tol.json).  Band
layout: [ch][iu = u + b][v = 0..b], complex; the half v < 0 is the conjugate mirror."""
import functools
from types import SimpleNamespace

import numpy as np

# (h, w, b): the shapes of the GPU tests; the last three sit at the width up to which the kernels
# table the x twiddles in LDS (4096: the table, whole groups of four pixels) and just past it
# (4100: twiddles formed in place, whole groups; 4101: the same with a tail)
SHAPES = [(3, 3, 1), (5, 7, 2), (64, 96, 2), (37, 53, 3), (67, 131, 5), (130, 134, 64), (720, 1280, 7),
          (5, 4096, 2), (5, 4100, 2), (5, 4101, 2)]


def key(h, w, b):
    return f"{h}x{w}_b{b}"


def fda_fft(src, tgt, b, strength=1.0):
    """fp64 [H, W, 3], not clamped: fft2, fftshift of the amplitudes, the window
    [H//2-b : H//2+b+1, W//2-b : W//2+b+1] blended towards the target's, ifftshift, ifft2, real."""
    assert src.shape == tgt.shape
    h, w, _ = src.shape
    out = np.empty(src.shape, dtype=np.float64)
    for ch in range(3):
        fs = np.fft.fft2(src[..., ch].astype(np.float64))
        ft = np.fft.fft2(tgt[..., ch].astype(np.float64))
        amp, pha = np.fft.fftshift(np.abs(fs)), np.angle(fs)
        amp_t = np.fft.fftshift(np.abs(ft))
        win = (slice(h // 2 - b, h // 2 + b + 1), slice(w // 2 - b, w // 2 + b + 1))
        amp[win] = (1.0 - strength) * amp[win] + strength * amp_t[win]
        out[..., ch] = np.real(np.fft.ifft2(np.fft.ifftshift(amp) * np.exp(1j * pha)))
    return out


def _twiddle(k, n, dtype):
    """e^{2 pi i k / n} for integer k already reduced to [0, n): folded to (-n/2, n/2], the
    argument 2k/n formed in ``dtype``, cos / sin of pi times it rounded to ``dtype``."""
    k = np.asarray(k, dtype=np.int64)
    k = np.where(2 * k > n, k - n, k)
    arg = ((2 * k).astype(dtype) / dtype(n)).astype(np.float64)
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    return (np.cos(np.pi * arg) + 1j * np.sin(np.pi * arg)).astype(ctype)


def _mm(a, b):
    """a @ b by numpy's own loops: the same bits whatever BLAS and however many threads."""
    return np.einsum("ik,kj->ij", a, b)


def band_spectrum(img, b, dtype=np.float64):
    """(spec complex [3, 2b+1, b+1], amp_norm [3, 2b+1, b+1]): F(u,v) = sum_y sum_x img[y][x][ch]
    e^{-2 pi i (uy/h + vx/w)} over the band -- rows reduced over x first, then over y -- and
    |F| / (hw)."""
    h, w, _ = img.shape
    assert 1 <= b and 2 * b + 1 <= min(h, w)
    v, u = np.arange(b + 1), np.arange(-b, b + 1)
    tx = np.conj(_twiddle((np.arange(w)[:, None] * v[None, :]) % w, w, dtype))        # [w, b+1]
    ty = np.conj(_twiddle((u[:, None] * np.arange(h)[None, :]) % h, h, dtype))        # [2b+1, h]
    ctype = tx.dtype
    spec = np.empty((3, 2 * b + 1, b + 1), dtype=ctype)
    for ch in range(3):
        rows = _mm(img[..., ch].astype(dtype).astype(ctype), tx)                         # [h, b+1]
        spec[ch] = _mm(ty, rows)
    amp = (np.abs(spec) / dtype(h * w)).astype(dtype)
    return spec, amp


def apply_band(src, spec_src, amp_ref_norm, b, strength=1.0, dtype=np.float64):
    """[H, W, 3] in ``dtype``, not clamped: the kernels' apply from the source's band and the
    target's normalised amplitudes (of a target of any size)."""
    h, w, _ = src.shape
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    spec = spec_src.astype(ctype)
    hw = dtype(h * w)
    a_t = amp_ref_norm.astype(dtype) * hw
    a_s = np.abs(spec).astype(dtype)
    safe = np.where(a_s == 0, dtype(1), a_s)
    d = np.where(a_s == 0, (dtype(strength) * a_t).astype(ctype), (dtype(strength) * (a_t - a_s) / safe) * spec).astype(ctype)
    v, u = np.arange(b + 1), np.arange(-b, b + 1)
    ty = _twiddle((np.arange(h)[:, None] * u[None, :]) % h, h, dtype)                 # [h, 2b+1]
    tx = _twiddle((v[:, None] * np.arange(w)[None, :]) % w, w, dtype)                 # [b+1, w]
    scale = (np.where(v == 0, dtype(1), dtype(2)) / hw).astype(dtype)
    out = np.empty(src.shape, dtype=dtype)
    for ch in range(3):
        g = _mm(ty, d[ch]) * scale[None, :]                                            # [h, b+1]
        out[..., ch] = src[..., ch].astype(dtype) + np.real(_mm(g, tx)).astype(dtype)
    return out


def to_u8(x):
    """rint, then the clamp: the kernels' uint8 epilogue."""
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def band_floor(img, b):
    """min / median of the band amplitudes of ``img``: the phase of a vanishing coefficient is
    noise, in the oracle too, so the tests use inputs where this is not small."""
    amp = band_spectrum(img, b)[1]
    return float(amp.min() / np.median(amp))


# ------------------------------------------------------------------ inputs
def _scene(h, w, seed, level, swing, grain):
    """Smooth gradients and one slow wave per channel plus noise, so the low band carries real
    energy in every coefficient."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h) / max(h - 1, 1), np.arange(w) / max(w - 1, 1), indexing="ij")
    img = np.empty((h, w, 3), dtype=np.float64)
    for ch in range(3):
        gy, gx, ph = rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(0, 2 * np.pi)
        fy, fx = rng.uniform(0.5, 2.0), rng.uniform(0.5, 2.0)
        smooth = gy * (yy - 0.5) + gx * (xx - 0.5) + 0.5 * np.sin(2 * np.pi * (fy * yy + fx * xx) + ph)
        img[..., ch] = level[ch] + swing * smooth + grain * rng.standard_normal((h, w))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def source(h=64, w=96, seed=1):
    """Dark, bluish (a rendered frame at dusk)."""
    return _scene(h, w, seed, level=(70, 80, 100), swing=30.0, grain=12.0)


def reference(h=37, w=53, seed=2):
    """Bright, warm, flatter."""
    return _scene(h, w, seed, level=(175, 160, 140), swing=18.0, grain=8.0)


def noise(h, w, seed=3):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def pair(h, w):
    """The (source, target) of one test shape, both h x w."""
    return source(h, w, seed=1000 + 7 * h + w), reference(h, w, seed=2000 + 7 * h + w)


# ------------------------------------------------------------------ shared results
@functools.lru_cache(maxsize=None)
def case(h, w, b):
    """Per test shape, computed once and left unchanged: the pair, the oracle, both restatements
    (s: the source's band, a: its normalised amplitudes, t: the target's) and the FFT's band."""
    src, tgt = pair(h, w)
    s64, _ = band_spectrum(src, b)
    _, t64 = band_spectrum(tgt, b)
    s32, a32 = band_spectrum(src, b, np.float32)
    _, t32 = band_spectrum(tgt, b, np.float32)
    band = np.stack([np.fft.fft2(src[..., ch].astype(np.float64))[np.arange(-b, b + 1)[:, None] % h, np.arange(b + 1)[None, :]]
                     for ch in range(3)])
    return SimpleNamespace(src=src, tgt=tgt, oracle=fda_fft(src, tgt, b), s64=s64, t64=t64, s32=s32, a32=a32, t32=t32, band=band,
                           out64=apply_band(src, s64, t64, b), out32=apply_band(src, s32, t32, b, 1.0, np.float32))


def spectrum_errors(spec, amp, band, h, w):
    """(max |spec - band|, max |amp - |band| / hw|), each relative to its channel's largest value."""
    top = np.abs(band).reshape(3, -1).max(1)[:, None, None]
    return float((np.abs(spec - band) / top).max()), float((np.abs(amp - np.abs(band) / (h * w)) / (top / (h * w))).max())
