"""The arithmetic contract of ``sgn_gt_downscale`` (include/sgn_rast.h, csrc/gt_pyramid.hip) restated in numpy fp32,
operation for operation: every intermediate is a float32 array and every ``*``, ``+``, ``-``, ``/`` one rounded numpy
operation (numpy never fuses a multiply into an add).  It is the documented definition, nothing more: the tests hold it
against ``torch.nn.functional.interpolate`` on the CPU (test_pyramid_oracle.py) and the kernel against it, bit for bit
(test_gpu_pyramid.py)."""
import numpy as np

F32 = np.float32


def bilinear_axis(inn: int, out: int):
    """(i0, i1, l0, l1) of the ``out`` destination indices of one axis of length ``inn``."""
    scale = F32(inn) / F32(out)
    dst = np.arange(out, dtype=F32)
    src = np.maximum(scale * (dst + F32(0.5)) - F32(0.5), F32(0.0))
    i0 = np.minimum(src.astype(np.int32), np.int32(inn - 1))
    i1 = i0 + (i0 < inn - 1).astype(np.int32)
    l1 = src - i0.astype(F32)
    l0 = F32(1.0) - l1
    assert src.dtype == l0.dtype == l1.dtype == F32
    return i0, i1, l0, l1


def nearest_axis(inn: int, out: int):
    scale = F32(inn) / F32(out)
    dst = np.arange(out, dtype=F32)
    return np.minimum(np.floor(dst * scale).astype(np.int32), np.int32(inn - 1))


def image(img: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """uint8 [h,w,3] -> float32 [oh,ow,3]."""
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
    h, w = img.shape[:2]
    q = img.astype(F32) / F32(255.0)                             # the correctly rounded u / 255 of every byte
    h0, h1, l0h, l1h = bilinear_axis(h, oh)
    w0, w1, l0w, l1w = bilinear_axis(w, ow)
    l0h, l1h = l0h[:, None, None], l1h[:, None, None]
    l0w, l1w = l0w[None, :, None], l1w[None, :, None]
    a, b = q[h0][:, w0], q[h0][:, w1]
    c, d = q[h1][:, w0], q[h1][:, w1]
    out = l0h * (l0w * a + l1w * b) + l1h * (l0w * c + l1w * d)
    assert out.dtype == F32
    return out


def nearest(m: np.ndarray, oh: int, ow: int) -> np.ndarray:
    """[h,w] or [h,w,1] of any dtype -> [oh,ow] or [oh,ow,1]: the source elements, unchanged."""
    h, w = m.shape[:2]
    return m[nearest_axis(h, oh)][:, nearest_axis(w, ow)]
