"""CPU: ``tests/frames_oracle.py`` — the float32 restatement the frame-packing kernel is held to — against nerfstudio's
own expressions, written out inline in torch (``apply_depth_colormap`` -> ``apply_colormap`` -> ``apply_float_colormap``,
as the reference's ``scripts/render.py:159-273`` calls them) and followed by the writers' float -> uint8 conversion
``(clip(a, 0, 1) * 255 + 0.5).astype(uint8)``.  Equal bytes, no tolerance.  (nerfstudio and the writer libraries are not
installed: the expressions are as recalled — unpinned.)"""
import numpy as np
import pytest
import torch

import frames_oracle as FO

PLANES = [(0.0, 3.0), (0.5, 77.3), (2.0, 2.0), (1e-3, 1e3)]
N = 200_000


def writer_bytes(a):
    """What an image / video writer makes of a float image."""
    a = np.asarray(a)
    assert a.dtype == np.float32
    return (np.clip(a, 0, 1) * 255 + 0.5).astype(np.uint8)


def ns_float_colormap_index(image, invert, nan_first=True):
    """``apply_colormap``'s default path (``normalize=False``, ``colormap_min=0``, ``colormap_max=1``) down to the index
    ``apply_float_colormap`` gathers with.  ``nan_first``: NaN -> 0 ahead of the inversion, the order the contract of
    ``sgn_frames_pack`` fixes; ``False`` swaps the two steps (they commute unless the input holds NaN)."""
    output = image * (1.0 - 0.0) + 0.0
    output = torch.clip(output, 0, 1)
    if nan_first:
        output = torch.nan_to_num(output, 0)
    if invert:
        output = 1 - output
    if not nan_first:
        output = torch.nan_to_num(output, 0)
    return (output * 255).long()


def ns_colormap(image, table, invert=False, nan_first=True):
    """``apply_colormap``: a three-channel image unchanged, a one-channel one through the float table [256,3]."""
    if image.shape[-1] == 3:
        return image
    idx = ns_float_colormap_index(image, invert, nan_first)
    assert int(idx.min()) >= 0 and int(idx.max()) <= 255      # apply_float_colormap's own assertions
    return table[idx[..., 0]]


def ns_depth_colormap(depth, near, far, table, invert=False, nan_first=True):
    """``apply_depth_colormap`` with both planes given."""
    depth = (depth - near) / (far - near + 1e-10)
    depth = torch.clip(depth, 0, 1)
    return ns_colormap(depth, table, invert, nan_first)


@pytest.fixture(scope="module")
def values():
    g = torch.Generator().manual_seed(0)
    v = torch.rand(N, generator=g) * 80.0 - 5.0               # -5 .. 75
    v[::1000] = float("nan")
    v[1::1000] = float("inf")
    v[2::1000] = float("-inf")
    v[3::1000] = 0.0
    v[4::1000] = -0.0
    return v.reshape(-1, 100, 1)


def random_table():
    return torch.rand(256, 3, generator=torch.Generator().manual_seed(5)) * 1.2 - 0.1     # some entries outside [0, 1]


def gray_float_table():
    return (torch.arange(256, dtype=torch.float32) / 255.0)[:, None].repeat(1, 3)


def tables():
    out = [("random", random_table()), ("gray", gray_float_table())]
    return out


@pytest.mark.parametrize("near,far", PLANES)
@pytest.mark.parametrize("invert", [False, True])
def test_depth_panels_equal_nerfstudio_then_the_writer(values, near, far, invert):
    from sgn_rast import frames
    lo, den = FO.planes(near, far)
    assert den == np.float32(far - near + 1e-10) and den != 0
    for name, table in tables():
        want = writer_bytes(ns_depth_colormap(values, near, far, table, invert).numpy())
        got = FO.scalar(values.numpy(), lo, den, invert, frames.byte_lut(table).numpy())
        assert got.shape == want.shape == values.shape[:2] + (3,)
        assert np.array_equal(got, want), (name, near, far, invert)
        assert np.array_equal(FO.panel(values.numpy(), near, far, invert, frames.byte_lut(table).numpy()), want)
    # the index alone, as the issue's own check had it
    t = torch.clip((values - near) / (far - near + 1e-10), 0, 1)
    idx = ns_float_colormap_index(t, invert)[..., 0].numpy()
    assert np.array_equal(FO.scalar_index(values.numpy()[..., 0], lo, den, invert), idx)
    assert idx.min() == 0 and idx.max() == 255


@pytest.mark.parametrize("invert", [False, True])
def test_accumulation_panels_equal_apply_colormap(invert):
    """``lo = 0, den = 1`` is apply_colormap's default path bit for bit: ``(x - 0) / 1`` and ``x * (1 - 0) + 0`` are x."""
    from sgn_rast import frames
    g = torch.Generator().manual_seed(1)
    x = torch.rand(300, 200, 1, generator=g) * 1.4 - 0.2
    x.view(-1)[:7] = torch.tensor([float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 1.0, 1e-40])
    k = torch.arange(256, dtype=torch.float32) / 255.0        # the index boundaries and their neighbours
    x.view(-1)[100:100 + 768] = torch.cat([k, torch.nextafter(k, k + 1), torch.nextafter(k, k - 1)])
    for name, table in tables():
        want = writer_bytes(ns_colormap(x, table, invert).numpy())
        lo, den = FO.planes(0.0, 1.0)
        assert lo == 0 and den == 1
        assert np.array_equal(FO.scalar(x.numpy(), lo, den, invert, frames.byte_lut(table).numpy()), want), name


def test_nan_to_zero_and_inversion_commute_without_nan(values):
    """The contract puts NaN -> 0 ahead of the inversion.  On inputs without NaN the other order gives the same index; a
    NaN under ``invert`` is row 255 in the contract's order (and row 0 in the other)."""
    clean = torch.nan_to_num(values, nan=1.25)
    for near, far in PLANES:
        a = ns_depth_colormap(clean, near, far, random_table(), True, nan_first=True)
        b = ns_depth_colormap(clean, near, far, random_table(), True, nan_first=False)
        assert torch.equal(a, b)
    nan = np.full((1, 1), np.nan, dtype=np.float32)
    assert FO.scalar_index(nan, 0.0, 1.0, False)[0, 0] == 0 and FO.scalar_index(nan, 0.0, 1.0, True)[0, 0] == 255


def test_rgb_panels_equal_the_writer():
    """apply_colormap returns a three-channel image unchanged; the writer quantises it.  numpy's cast of NaN to uint8 is
    not defined, so NaN is held to the contract's own rule (NaN -> 0) and everything else to the writer."""
    g = torch.Generator().manual_seed(2)
    x = torch.rand(200, 301, 3, generator=g) * 1.6 - 0.3
    k = (torch.arange(256, dtype=torch.float32) + 0.5) / 255.0   # the rounding boundaries and their neighbours
    edge = torch.cat([k, torch.nextafter(k, k + 1), torch.nextafter(k, k - 1),
                      torch.tensor([0.0, -0.0, 1.0, 1e-40, -1e-40, float("inf"), float("-inf"), 2.0, -3.0])])
    x.view(-1)[:edge.numel()] = edge
    img = ns_colormap(x, None)
    assert img is x
    assert np.array_equal(FO.rgb(x.numpy()), writer_bytes(img.numpy()))
    assert np.array_equal(FO.panel(x.numpy()), writer_bytes(img.numpy()))
    special = FO.q(np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, 0.5], dtype=np.float32))
    assert special.tolist() == [0, 255, 0, 0, 255, 128]


def test_bytes_panels_are_copied():
    x = np.arange(256 * 3, dtype=np.uint8).reshape(16, 16, 3)
    out = FO.panel(x)
    assert np.array_equal(out, x) and out is not x


def test_byte_lut_and_the_gray_table():
    from sgn_rast import frames
    table = random_table()
    lut = frames.byte_lut(table)
    assert lut.dtype == torch.uint8 and tuple(lut.shape) == (256, 3) and lut.device.type == "cpu"
    assert np.array_equal(lut.numpy(), FO.q(table.numpy()))
    assert np.array_equal(lut.numpy(), writer_bytes(table.numpy()))
    assert np.array_equal(frames.byte_lut(table.numpy()).numpy(), lut.numpy())        # array-likes are taken
    assert np.array_equal(frames.byte_lut(table.double().tolist()).numpy(), lut.numpy())
    nan_row = table.clone()
    nan_row[3, 1] = float("nan")
    assert int(frames.byte_lut(nan_row)[3, 1]) == 0
    gray = frames.colormap("gray", device="cpu")
    assert gray.dtype == torch.uint8 and np.array_equal(gray.numpy(), FO.gray_table())
    assert np.array_equal(frames.byte_lut(gray_float_table()).numpy(), FO.gray_table())   # row i is i / 255: byte i
    assert frames.colormap("gray", device="cpu") is gray                                   # cached per (name, device)
    with pytest.raises(ValueError):
        frames.byte_lut(torch.zeros(255, 3))
    with pytest.raises(ValueError):
        frames.byte_lut(torch.zeros(256, 4))
    with pytest.raises(TypeError):
        frames.byte_lut("turbo")


def test_turbo_through_matplotlib(values):
    matplotlib = pytest.importorskip("matplotlib")
    from sgn_rast import frames
    table = torch.tensor(matplotlib.colormaps["turbo"].colors)      # as apply_float_colormap builds it
    assert table.dtype == torch.float32 and tuple(table.shape) == (256, 3)
    lut = frames.colormap("default", device="cpu")
    assert lut is frames.colormap("turbo", device="cpu")
    assert np.array_equal(lut.numpy(), writer_bytes(table.numpy()))
    for near, far in PLANES:
        lo, den = FO.planes(near, far)
        want = writer_bytes(ns_depth_colormap(values, near, far, table).numpy())
        assert np.array_equal(FO.scalar(values.numpy(), lo, den, False, lut.numpy()), want)
    with pytest.raises(ValueError):
        frames.colormap("no-such-colour-map", device="cpu")
