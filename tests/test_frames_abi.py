"""CPU: ``sgn_frames_pack`` (include/sgn_rast.h, "A frame's eval outputs as the bytes ...") is exported, declared and in
the ctypes table; it rejects each bad argument with its return code before touching the device; and
``sgn_rast.frames.pack`` / ``Panel`` / ``FrameSink`` raise every host-side ``TypeError`` / ``ValueError`` before the
library's device check, which CPU tensors then fail (no quiet CPU path)."""
import ctypes
import os

import pytest
import torch

from sgn_rast import _lib

NAME = "sgn_frames_pack"
F = 0x1000      # never dereferenced: every case below fails its argument check first
RGB, SCALAR, BYTES = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsgnrast.so is not built (run __graft_entry__.build())")
    return _lib.load()


def test_entry_is_exported_and_declared(lib):
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 8
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sgn_rast.h")).read()
    assert "int sgn_frames_pack(int h, int w, int n_panels, const sgn_panel *panels" in header
    assert "typedef struct sgn_panel {" in header and "#define SGN_FRAMES_MAX_PANELS 16" in header
    # the ctypes struct is the header's, field for field: two pointers, four int32, two floats
    assert ctypes.sizeof(_lib.PanelDesc) == 40
    assert [f[0] for f in _lib.PanelDesc._fields_] == ["src", "lut", "kind", "y0", "x0", "invert", "lo", "den"]
    assert (_lib.PANEL_RGB, _lib.PANEL_SCALAR, _lib.PANEL_BYTES, _lib.FRAMES_MAX_PANELS) == (0, 1, 2, 16)
    from sgn_rast import frames
    import sgn_rast
    for name in ("FrameSink", "Panel", "byte_lut", "colormap", "pack"):
        assert getattr(sgn_rast, name) is getattr(frames, name)


def _panel(kind=RGB, y0=0, x0=0, src=F, lut=F, lo=0.0, den=1.0, invert=0):
    return dict(kind=kind, y0=y0, x0=x0, src=src, lut=lut, lo=lo, den=den, invert=invert)


def _call(lib, panels=None, h=8, w=12, canvas=F, canvas_h=32, canvas_w=40, n_panels=None, null_panels=False):
    panels = [_panel()] if panels is None else panels
    table = (_lib.PanelDesc * max(len(panels), 1))()
    for d, p in zip(table, panels):
        for k, v in p.items():
            setattr(d, k, v)
    n = len(panels) if n_panels is None else n_panels
    return lib.sgn_frames_pack(h, w, n, None if null_panels else table, canvas, canvas_h, canvas_w, None)


def test_geometry_errors(lib):
    column = lambda n, **kw: [_panel(y0=8 * i, **kw) for i in range(n)]
    for kw in (dict(h=0), dict(w=0), dict(h=-3), dict(canvas_h=0), dict(canvas_w=-1),
               dict(h=16385, canvas_h=16385), dict(w=16385, canvas_w=16385), dict(canvas_h=16385), dict(canvas_w=16385),
               dict(n_panels=0), dict(n_panels=-1), dict(n_panels=17), dict(panels=column(17), canvas_h=8 * 17),
               dict(panels=[_panel(kind=3)]), dict(panels=[_panel(kind=-1)]),
               dict(panels=[_panel(y0=-1)]), dict(panels=[_panel(x0=-1)]),
               dict(panels=[_panel(y0=25)]), dict(panels=[_panel(x0=29)]),           # 25 + 8 > 32, 29 + 12 > 40
               dict(panels=[_panel(), _panel(y0=24, x0=28), _panel(y0=7, x0=11)]),   # the third overlaps the first
               dict(panels=[_panel(), _panel()]),
               dict(panels=[_panel(kind=SCALAR, den=0.0)]), dict(panels=[_panel(kind=SCALAR, den=-0.0)]),
               dict(panels=[_panel(kind=SCALAR, den=float("inf"))]), dict(panels=[_panel(kind=SCALAR, den=float("nan"))]),
               dict(panels=[_panel(kind=SCALAR, den=float("-inf"))])):
        assert _call(lib, **kw) == -1, kw
        assert NAME.encode() in lib.sgn_last_error()
    assert _call(lib, h=0, canvas=None) == -1                  # the sizes are reported first
    assert _call(lib, n_panels=17, null_panels=True) == -1


def test_pointer_errors(lib):
    for kw in (dict(null_panels=True), dict(canvas=None), dict(panels=[_panel(src=None)]),
               dict(panels=[_panel(), _panel(y0=8, src=None)]),
               dict(panels=[_panel(kind=SCALAR, lut=None)]), dict(panels=[_panel(kind=BYTES, src=None, lut=None)]),
               dict(h=16384, w=16384, canvas_h=16384, canvas_w=16384, canvas=None)):
        assert _call(lib, **kw) == -2, kw
        assert NAME.encode() in lib.sgn_last_error()
    # a colour table is asked of SCALAR panels only; den is looked at for SCALAR panels only: these pass every check
    # up to the pointers, which is where the probe stops them
    assert _call(lib, panels=[_panel(kind=RGB, lut=None, den=0.0, src=None)]) == -2
    assert _call(lib, panels=[_panel(kind=BYTES, lut=None, den=float("nan"), src=None)]) == -2
    # 16 panels, touching but not overlapping, fill the canvas exactly
    grid = [_panel(kind=i % 3, y0=8 * (i // 4), x0=12 * (i % 4), src=None) for i in range(16)]
    assert _call(lib, panels=grid, canvas_h=32, canvas_w=48) == -2


# ------------------------------------------------------------------------------------------------ host-side errors
H, W = 6, 10


def _outputs():
    g = torch.Generator().manual_seed(0)
    return {"rgb": torch.rand(H, W, 3, generator=g), "depth": torch.rand(H, W, 1, generator=g) * 50,
            "acc": torch.rand(H, W, generator=g), "gt": torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g)}


def _panels(frames):
    return [frames.Panel("rgb"), frames.Panel("depth", 0.5, 77.3, lut="gray"), frames.Panel("acc", lut="gray"),
            frames.Panel("gt")]


def test_panel_errors():
    from sgn_rast import frames
    for kw in (dict(name=3), dict(name=None), dict(near="0"), dict(far=None), dict(near=True), dict(invert="yes"),
               dict(invert=2), dict(lut=7), dict(lut=None), dict(lut=torch.zeros(256, 3)),
               dict(lut=torch.zeros(256, 3, dtype=torch.int32))):
        with pytest.raises(TypeError):
            frames.Panel(**{"name": "depth", **kw})
    for kw in (dict(near=float("nan")), dict(far=float("inf")), dict(near=float("-inf")),
               dict(near=1e-10, far=0.0),                       # far - near + 1e-10 == 0
               dict(near=0.0, far=-1e-10),
               dict(near=0.0, far=1e39),                        # the denominator does not fit fp32
               dict(near=-3e38, far=3e38),
               dict(lut=torch.zeros(255, 3, dtype=torch.uint8)), dict(lut=torch.zeros(256, 4, dtype=torch.uint8))):
        with pytest.raises(ValueError):
            frames.Panel(**{"name": "depth", **kw})
    p = frames.Panel("depth", 2, 2)                             # near == far: the 1e-10 keeps the denominator alive
    assert p.lo == 2.0 and 0 < p.den < 2e-10 and not p.invert and p.lut == "default"
    assert frames.Panel("d", 0.5, 77.3).den == float(torch.tensor(77.3 - 0.5 + 1e-10, dtype=torch.float64).float())


def test_pack_type_errors():
    from sgn_rast import frames
    out, panels = _outputs(), _panels(frames)
    assert not issubclass(_lib.SgnRastError, (TypeError, ValueError))
    for bad in (dict(out, rgb=out["rgb"].double()), dict(out, rgb=out["rgb"].half()), dict(out, rgb=out["rgb"].numpy()),
                dict(out, gt=out["gt"].to(torch.int32)), dict(out, acc=out["acc"] > 0.5), dict(out, depth=None),
                [out["rgb"]], out["rgb"], None):
        with pytest.raises(TypeError):
            frames.pack(bad, panels)
    for bad in ("rgb", frames.Panel("rgb"), ["rgb"], [frames.Panel("rgb"), "depth"], None, 3, {"rgb": frames.Panel("rgb")}):
        with pytest.raises(TypeError):
            frames.pack(out, bad)
    for bad in (torch.zeros(4 * H, W, 3), torch.zeros(4 * H, W, 3, dtype=torch.int8), "canvas"):
        with pytest.raises(TypeError):
            frames.pack(out, panels, out=bad)


def test_pack_value_errors():
    from sgn_rast import frames
    out, panels = _outputs(), _panels(frames)
    for bad in (dict(out, rgb=out["rgb"][..., :2]), dict(out, rgb=out["rgb"][None]), dict(out, rgb=out["rgb"][..., 0, 0]),
                dict(out, gt=out["gt"][..., 0]), dict(out, gt=out["gt"][..., :1]), dict(out, depth=out["depth"][None]),
                dict(out, depth=out["depth"].expand(H, W, 2)), dict(out, acc=out["acc"][:0]),
                dict(out, acc=out["acc"][:-1]), dict(out, depth=out["depth"][:, :-1]), dict(out, gt=out["gt"][1:]),
                {k: v for k, v in out.items() if k != "depth"}, {}):
        with pytest.raises(ValueError):
            frames.pack(bad, panels)
    with pytest.raises(ValueError):
        frames.pack(out, [])
    with pytest.raises(ValueError):
        frames.pack(out, [frames.Panel("rgb"), frames.Panel("rgb")])            # the names key the views
    many = {f"p{i}": out["acc"] for i in range(17)}
    with pytest.raises(ValueError):
        frames.pack(many, [frames.Panel(k, lut="gray") for k in many])
    for arrange in ("grid", "", None, 0):
        with pytest.raises(ValueError):
            frames.pack(out, panels, arrange=arrange)
    wide = {"a": torch.zeros(1, 9000), "b": torch.zeros(1, 9000)}              # 2 x 9000 > 16384 in a row
    with pytest.raises(ValueError):
        frames.pack(wide, [frames.Panel("a", lut="gray"), frames.Panel("b", lut="gray")], arrange="row")
    with pytest.raises(ValueError):
        frames.pack({"a": torch.zeros(1, 16385)}, [frames.Panel("a", lut="gray")])
    for bad in (torch.zeros(4 * H, W, 4, dtype=torch.uint8), torch.zeros(H, 4 * W, 3, dtype=torch.uint8),
                torch.zeros(4 * H, 2 * W, 3, dtype=torch.uint8)[:, ::2]):
        with pytest.raises(ValueError):
            frames.pack(out, panels, out=bad)


def test_an_unknown_colour_map_is_a_value_error():
    pytest.importorskip("matplotlib")
    from sgn_rast import frames
    with pytest.raises(ValueError):
        frames.pack(_outputs(), [frames.Panel("acc", lut="no-such-colour-map")])
    with pytest.raises(ValueError):
        frames.pack(_outputs(), [frames.Panel("acc", lut="jet")])      # not a listed map: no 256-row table
    frames.Panel("rgb", lut="no-such-colour-map")                      # a name is resolved only where a table is needed
    with pytest.raises(_lib.SgnRastError):
        frames.pack(_outputs(), [frames.Panel("rgb", lut="no-such-colour-map")])


def test_sink_errors():
    from sgn_rast import frames
    panels = _panels(frames)
    for kw in (dict(panels="rgb"), dict(panels=[1]), dict(height=2.5), dict(width="7"), dict(height=True),
               dict(slots=2.0), dict(slots=None), dict(slots=True), dict(on_frame=3)):
        with pytest.raises(TypeError):
            frames.FrameSink(**{"panels": panels, "height": H, "width": W, **kw})
    for kw in (dict(panels=[]), dict(panels=panels * 5), dict(height=0), dict(width=-4), dict(width=16385),
               dict(height=5000), dict(width=5000, arrange="row"), dict(arrange="grid"), dict(slots=1), dict(slots=0),
               dict(device="cpu")):
        with pytest.raises(ValueError):
            frames.FrameSink(**{"panels": panels, "height": H, "width": W, **kw})
    sink = frames.FrameSink(panels, H, W, arrange="row", slots=3)      # the constructor allocates nothing
    assert sink.canvas_shape == (H, 4 * W, 3) and len(sink) == 0
    assert sink.drain() == [] and sink.poll() == 0                     # nothing outstanding: no device work either
    out = _outputs()
    with pytest.raises(TypeError):
        sink.submit(dict(out, rgb=out["rgb"].double()))
    with pytest.raises(ValueError):
        sink.submit({k: v[:-1] for k, v in out.items()})               # not the sink's size
    with pytest.raises(ValueError):
        sink.submit({k: v for k, v in out.items() if k != "gt"})
    with pytest.raises(_lib.SgnRastError):
        sink.submit(out)                                               # CPU tensors: the device check, before allocating
    with sink:
        pass


def test_cpu_tensors_reach_the_device_check():
    """No quiet CPU path; a bad argument is still reported first."""
    from sgn_rast import frames
    out, panels = _outputs(), _panels(frames)
    for arrange in ("column", "row"):
        with pytest.raises(_lib.SgnRastError):
            frames.pack(out, panels, arrange=arrange)
    with pytest.raises(_lib.SgnRastError):
        frames.pack(out, panels[:1])
    with pytest.raises(_lib.SgnRastError):
        frames.pack(out, panels, out=torch.zeros(4 * H, W, 3, dtype=torch.uint8))
    with pytest.raises(_lib.SgnRastError):
        frames.pack(out, [frames.Panel("acc", lut=torch.zeros(256, 3, dtype=torch.uint8))])
    with pytest.raises(TypeError):
        frames.pack(dict(out, rgb=out["rgb"].double()), panels)


def test_a_missing_matplotlib_is_an_import_error(monkeypatch):
    """Any table but "gray" is looked up in matplotlib on first use; without it the error says so, before device work."""
    import sys
    from sgn_rast import frames
    monkeypatch.setitem(sys.modules, "matplotlib", None)            # `import matplotlib` raises ImportError
    monkeypatch.setattr(frames, "_tables", {})
    with pytest.raises(ImportError, match="matplotlib"):
        frames.colormap("viridis", device="cpu")
    with pytest.raises(ImportError, match="matplotlib"):
        frames.pack(_outputs(), [frames.Panel("acc")])              # lut="default" -> "turbo"
    assert tuple(frames.colormap("gray", device="cpu").shape) == (256, 3)
