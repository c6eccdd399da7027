"""numpy restatement of ``sgn_frames_pack`` (include/sgn_rast.h, "A frame's eval outputs as the bytes ..."): the writers'
quantiser and the three panel kinds, in float32 with the contract's operation order, every operation rounded on its own.
``tests/test_frames_oracle.py`` holds it to nerfstudio's expressions; the GPU tests hold the kernel to it, bit for bit."""
import numpy as np

F = np.float32


def q(x):
    """float -> uint8 as the writers do it: ``c = x`` clamped to [0, 1] (NaN -> 0, -inf -> 0, +inf -> 1),
    ``trunc(c * 255 + 0.5)``."""
    x = np.asarray(x, dtype=F)
    c = np.where(x > 0, np.where(x < 1, x, F(1)), F(0)).astype(F)
    v = c * F(255.0)
    v = v + F(0.5)
    assert v.dtype == F
    return v.astype(np.uint8)                      # 0.5 .. 255.5: truncation


def rgb(x):
    """``RGB``: float32 [h,w,3] -> uint8 [h,w,3]."""
    x = np.asarray(x, dtype=F)
    assert x.ndim == 3 and x.shape[2] == 3
    return q(x)


def planes(near, far):
    """``(lo, den)`` as the host forms them: ``(float) near`` and ``(float)((double) far - (double) near + 1e-10)``."""
    return F(near), F(float(far) - float(near) + 1e-10)


def scalar_index(x, lo, den, invert):
    """The table row of every pixel: ``t = (x - lo) / den``; clip (NaN propagates); NaN -> 0; ``1 - t`` if invert;
    ``trunc(t * 255)``."""
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        t = (x - F(lo)) / F(den)
        assert t.dtype == F
        t = np.clip(t, F(0), F(1))
        t = np.where(np.isnan(t), F(0), t).astype(F)
        if invert:
            t = F(1) - t
        v = t * F(255.0)
    assert v.dtype == F
    return v.astype(np.int32)


def scalar(x, lo, den, invert, lut):
    """``SCALAR``: float32 [h,w] or [h,w,1] -> uint8 [h,w,3] through ``lut`` uint8 [256,3]."""
    x = np.asarray(x, dtype=F)
    x = x[..., 0] if x.ndim == 3 else x
    lut = np.asarray(lut)
    assert lut.dtype == np.uint8 and lut.shape == (256, 3)
    return lut[scalar_index(x, lo, den, invert)]


def copy(x):
    """``BYTES``: uint8 [h,w,3], unchanged."""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim == 3 and x.shape[2] == 3
    return x.copy()


def gray_table():
    return np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)


def panel(x, near=0.0, far=1.0, invert=False, lut=None):
    """One panel by the rule of ``frames.Panel``: the kind follows from the array."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return copy(x)
    if x.ndim == 3 and x.shape[2] == 3:
        return rgb(x)
    lo, den = planes(near, far)
    return scalar(x, lo, den, invert, lut)
