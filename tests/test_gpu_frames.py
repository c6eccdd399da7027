"""GPU (-m gpu): ``sgn_frames_pack`` / ``sgn_rast.frames`` on the HIP kernel against ``tests/frames_oracle.py``.  Every
comparison is ``torch.equal``: the arithmetic is a contract, there is no tolerance.  Values are placed on both sides of
every rounding and index boundary; every canvas is pre-filled with 0xAB and larger than what is written, and every byte
outside the panels must still be 0xAB afterwards."""
import ctypes

import numpy as np
import pytest
import torch

import frames_oracle as FO

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = 0xAB
SIZES = [(1, 1), (1, 3), (3, 5), (7, 4), (23, 37), (16, 64), (33, 129), (1280, 1920)]
PLANES = [(0.0, 1.0), (0.0, 3.0), (0.5, 77.3), (2.0, 2.0)]
SPECIAL = [0.0, -0.0, 1.0, -0.25, -7.0, 1.5, 300.0, 1e-40, -1e-40, float("nan"), float("inf"), float("-inf")]


# ------------------------------------------------------------------------------------------------ deliberate values
def _both_sides(v):
    v = np.asarray(v, dtype=np.float32)
    return np.concatenate([v, np.nextafter(v, np.float32(np.inf)), np.nextafter(v, np.float32(-np.inf))])


def _fill(shape, edge, seed, lo, hi):
    """float32 array of `shape`: the deliberate values first (rolled by the seed, so that small shapes do not all see the
    same few), seeded random values in lo..hi behind them."""
    n = int(np.prod(shape))
    rnd = np.random.default_rng(seed).uniform(lo, hi, size=n).astype(np.float32)
    edge = np.roll(np.asarray(edge, dtype=np.float32), -7 * seed)
    m = min(n, edge.size)
    rnd[:m] = edge[:m]
    if n > 4 * edge.size:                                      # and once more away from the row starts
        rnd[-edge.size - 5:-5] = edge
    return rnd.reshape(shape)


def rgb_values(h, w, seed=0):
    """Both sides of every rounding boundary (k + 0.5) / 255 of the quantiser, and the special values."""
    k = (np.arange(256, dtype=np.float32) + np.float32(0.5)) / np.float32(255.0)
    return _fill((h, w, 3), np.concatenate([np.asarray(SPECIAL, np.float32), _both_sides(k)]), seed, -0.3, 1.3)


def scalar_values(h, w, near, far, seed=0, trailing=False):
    """Both sides of every index boundary k / 255 mapped back through the planes, the middle of every index's interval
    (so that every table row is hit whatever the roundings at the boundaries do), and the special values: 1038 values, at
    a size with fewer pixels as many as fit."""
    lo, den = FO.planes(near, far)
    k = (np.arange(256, dtype=np.float64) / 255.0) * float(den) + float(lo)
    mid = ((np.arange(255, dtype=np.float64) + 0.5) / 255.0) * float(den) + float(lo)
    edge = np.concatenate([np.asarray(SPECIAL, np.float32), np.asarray([near, far, far + abs(far)], np.float32),
                           _both_sides(k.astype(np.float32)), mid.astype(np.float32)])
    span = max(far - near, 1.0)
    return _fill((h, w, 1) if trailing else (h, w), edge, seed, near - 0.2 * span, far + 0.2 * span)


def byte_values(h, w, seed=0):
    n = h * w * 3
    v = np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)
    m = min(n, 256)
    v[:m] = np.roll(np.arange(256, dtype=np.uint8), -11 * seed)[:m]            # every byte value present
    return v.reshape(h, w, 3)


@pytest.fixture(scope="module")
def luts():
    """(name, numpy, device tensor): a seeded random table and the gray table."""
    from sgn_rast import frames
    rnd = np.random.default_rng(42).integers(0, 256, size=(256, 3), dtype=np.uint8)
    gray = frames.colormap("gray", DEV)
    assert np.array_equal(gray.cpu().numpy(), FO.gray_table())
    return [("random", rnd, torch.from_numpy(rnd).to(DEV)), ("gray", FO.gray_table(), gray)]


def guarded(ch, cw, guard=256):
    """A [ch,cw,3] canvas inside a larger 0xAB buffer: (buffer, canvas view, guard)."""
    buf = torch.full((ch * cw * 3 + 2 * guard,), FILL, dtype=torch.uint8, device=DEV)
    return buf, buf[guard:guard + ch * cw * 3].view(ch, cw, 3), guard


def guards_intact(buf, guard):
    return bool((buf[:guard] == FILL).all()) and bool((buf[-guard:] == FILL).all())


def mixed_frame(h, w, luts, n_scalar=8, seed=0):
    """One frame with all three kinds: (outputs on the host as numpy, Panel kwargs per name, in canvas order)."""
    outs = {"rgb": rgb_values(h, w, seed), "gt": byte_values(h, w, seed), "rgb2": rgb_values(h, w, seed + 3)}
    spec = {"rgb": {}, "gt": {}, "rgb2": {}}
    order = ["rgb"]
    for i in range(n_scalar):
        near, far = PLANES[i % 4]
        invert = i >= 4
        name = f"s{i}"
        outs[name] = scalar_values(h, w, near, far, seed + i, trailing=bool(i % 2))
        spec[name] = dict(near=near, far=far, invert=invert, lut=luts[(i + i // 4) % 2])
        order.append(name)
    order += ["gt", "rgb2"]
    return outs, spec, order


def expected_panel(x, kw):
    if not kw:
        return FO.panel(x)
    return FO.panel(x, kw["near"], kw["far"], kw["invert"], kw["lut"][1])


def to_panels(frames, spec, order):
    return [frames.Panel(n, **({} if not spec[n] else dict(spec[n], lut=spec[n]["lut"][2]))) for n in order]


# ------------------------------------------------------------------------------------------------ pack, every size
@pytest.mark.parametrize("arrange", ["column", "row"])
@pytest.mark.parametrize("h,w", SIZES)
def test_pack_equals_the_oracle(luts, h, w, arrange):
    from sgn_rast import frames
    big = h * w > 100_000
    outs, spec, order = mixed_frame(h, w, luts, n_scalar=2 if big else 8, seed=h + w)
    if big:
        order = ["rgb", "s0", "s1", "gt"]                       # the production shape: one panel of each kind, two tables
    dev = {k: torch.from_numpy(outs[k]).to(DEV) for k in order}
    panels = to_panels(frames, spec, order)
    n = len(order)
    ch, cw = (n * h, w) if arrange == "column" else (h, n * w)
    buf, canvas, guard = guarded(ch, cw)
    got, views = frames.pack(dev, panels, arrange=arrange, out=canvas)
    assert got is canvas and list(views) == order
    want = np.concatenate([expected_panel(outs[k], spec[k]) for k in order], axis=0 if arrange == "column" else 1)
    assert torch.equal(canvas.cpu(), torch.from_numpy(want))
    assert guards_intact(buf, guard)
    for i, k in enumerate(order):
        assert tuple(views[k].shape) == (h, w, 3)
        assert torch.equal(views[k].cpu(), torch.from_numpy(expected_panel(outs[k], spec[k]))), k
    # a fresh canvas (out=None) holds the same bytes
    fresh, fviews = frames.pack(dev, panels, arrange=arrange)
    assert fresh.dtype == torch.uint8 and tuple(fresh.shape) == (ch, cw, 3) and torch.equal(fresh, canvas)
    assert fviews[order[-1]].data_ptr() == fresh[(n - 1) * h if arrange == "column" else 0:,
                                                 0 if arrange == "column" else (n - 1) * w:].data_ptr()


def test_deliberate_values_reach_both_paths():
    """What the value builders promise, checked on the oracle alone: every byte is produced by the RGB panel at a size of
    the quad path and at one of the byte path; every table row is hit (t == 1 hits row 255), with and without inversion,
    at the sizes that hold all 1038 scalar values: (33, 129) on the byte path, the production size on the quad path."""
    for h, w in ((16, 64), (23, 37)):
        assert set(np.unique(FO.rgb(rgb_values(h, w)))) == set(range(256))
        assert set(np.unique(byte_values(h, w))) == set(range(256))
    for (h, w), planes in (((33, 129), PLANES[:3]), ((1280, 1920), PLANES[2:3])):
        for near, far in planes:
            lo, den = FO.planes(near, far)
            x = scalar_values(h, w, near, far)
            for invert in (False, True):
                assert set(np.unique(FO.scalar_index(x, lo, den, invert))) == set(range(256)), (near, far, invert)
    assert FO.scalar_index(np.float32([[1.0]]), 0.0, 1.0, False)[0, 0] == 255
    lo, den = FO.planes(2.0, 2.0)                              # near == far: everything is row 0 or row 255
    assert set(np.unique(FO.scalar_index(scalar_values(16, 64, 2.0, 2.0), lo, den, False))) == {0, 255}


def test_unaligned_canvas_and_sources_take_the_byte_path(luts):
    """w % 4 == 0 and yet no quad is aligned: a canvas that starts on an odd byte, float sources 4 bytes off a 16-byte
    boundary, a byte source on an odd byte.  The same bytes."""
    from sgn_rast import frames
    h, w = 16, 64
    outs, spec, order = mixed_frame(h, w, luts, seed=5)

    def shifted(a):
        t = torch.from_numpy(a).to(DEV)
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        flat[1:].copy_(t.reshape(-1))
        return flat[1:].view(t.shape)

    for shift_src, guard in ((False, 1), (True, 256), (True, 3)):
        dev = {k: shifted(outs[k]) if shift_src else torch.from_numpy(outs[k]).to(DEV) for k in order}
        if shift_src:
            assert dev["rgb"].data_ptr() % 16 == 4 and dev["gt"].data_ptr() % 4 == 1 and dev["rgb"].is_contiguous()
        buf, canvas, guard = guarded(len(order) * h, w, guard)
        assert canvas.data_ptr() % 4 == guard % 4
        frames.pack(dev, to_panels(frames, spec, order), out=canvas)
        want = np.concatenate([expected_panel(outs[k], spec[k]) for k in order], axis=0)
        assert torch.equal(canvas.cpu(), torch.from_numpy(want))
        assert guards_intact(buf, guard)


def test_sixteen_panels_of_mixed_kinds(luts):
    from sgn_rast import frames
    for (h, w), arrange in (((16, 64), "row"), ((23, 37), "column")):
        outs, spec, order = mixed_frame(h, w, luts, n_scalar=8, seed=9)
        for i in range(5):                                     # 11 -> 16 panels
            name = f"extra{i}"
            outs[name] = (rgb_values, byte_values)[i % 2](h, w, 20 + i)
            spec[name] = {}
            order.insert(2 * i, name)
        assert len(order) == 16
        dev = {k: torch.from_numpy(outs[k]).to(DEV) for k in order}
        ch, cw = (16 * h, w) if arrange == "column" else (h, 16 * w)
        buf, canvas, guard = guarded(ch, cw)
        frames.pack(dev, to_panels(frames, spec, order), arrange=arrange, out=canvas)
        want = np.concatenate([expected_panel(outs[k], spec[k]) for k in order], axis=0 if arrange == "column" else 1)
        assert torch.equal(canvas.cpu(), torch.from_numpy(want))
        assert guards_intact(buf, guard)


# ------------------------------------------------------------------------------------------------ the C entry
def c_pack(h, w, placed, canvas):
    """`placed`: [(y0, x0, device tensor, Panel kwargs or {})] straight through sgn_frames_pack."""
    from sgn_rast import _lib as L
    table = (L.PanelDesc * len(placed))()
    for d, (y0, x0, t, kw) in zip(table, placed):
        d.src, d.y0, d.x0 = t.data_ptr(), y0, x0
        d.kind = L.PANEL_BYTES if t.dtype == torch.uint8 else (L.PANEL_RGB if t.dim() == 3 and t.shape[2] == 3
                                                              else L.PANEL_SCALAR)
        d.lo, d.den, d.invert = 0.0, 1.0, 0
        if kw:
            lo, den = FO.planes(kw["near"], kw["far"])
            d.lut, d.lo, d.den, d.invert = kw["lut"][2].data_ptr(), float(lo), float(den), int(kw["invert"])
    ch, cw = canvas.shape[:2]
    L.check(L.load().sgn_frames_pack(h, w, len(placed), table, canvas.data_ptr(), ch, cw, L.stream_ptr()),
            "sgn_frames_pack")


@pytest.mark.parametrize("h,w", [(3, 5), (7, 4), (16, 64), (33, 129)])
@pytest.mark.parametrize("canvas_pad", [0, 1, 2, 3])
def test_hand_made_canvas_through_the_c_entry(luts, h, w, canvas_pad):
    """Panels scattered over a canvas larger than their union: x0 % 4 in {0, 1, 2, 3}, canvas_w % 4 == canvas_pad.  With
    canvas_pad == 0 the panel at x0 % 4 == 0 takes the quad path next to neighbours on the byte path."""
    outs, spec, _ = mixed_frame(h, w, luts, n_scalar=8, seed=canvas_pad)
    # canvas order: column k % 4 of the grid below, so that a panel of each kind (gt, rgb, s6) sits at x0 % 4 == 0
    order = ["gt", "s0", "s1", "s2", "rgb", "s3", "s4", "s5", "s6", "s7", "rgb2"]
    cols = [c + (k - c % 4) % 4 for k, c in enumerate([4, w + 9, 2 * w + 14, 3 * w + 19])]
    assert [c % 4 for c in cols] == [0, 1, 2, 3] and all(b - a > w for a, b in zip(cols, cols[1:]))
    rows = [3, h + 6, 2 * h + 9]
    slots = [(y, x) for y in rows for x in cols][:len(order)]
    cw = cols[-1] + w + 5
    cw += (canvas_pad - cw % 4) % 4
    ch = rows[-1] + h + 2
    assert cw % 4 == canvas_pad
    canvas = torch.full((ch, cw, 3), FILL, dtype=torch.uint8, device=DEV)
    dev = {k: torch.from_numpy(outs[k]).to(DEV) for k in order}
    c_pack(h, w, [(y0, x0, dev[k], spec[k]) for (y0, x0), k in zip(slots, order)], canvas)
    want = np.full((ch, cw, 3), FILL, dtype=np.uint8)
    for (y0, x0), k in zip(slots, order):
        want[y0:y0 + h, x0:x0 + w] = expected_panel(outs[k], spec[k])
    assert torch.equal(canvas.cpu(), torch.from_numpy(want))                      # the panels, and 0xAB everywhere else


def test_the_c_entry_reports_errors_on_device_pointers_too(luts):
    from sgn_rast import _lib as L
    t = torch.zeros(4, 8, 3, device=DEV)
    canvas = torch.full((8, 8, 3), FILL, dtype=torch.uint8, device=DEV)
    with pytest.raises(L.SgnRastError, match="sgn_frames_pack"):
        c_pack(4, 8, [(0, 0, t, {}), (3, 0, t, {})], canvas)                      # overlap
    with pytest.raises(L.SgnRastError, match="sgn_frames_pack"):
        c_pack(4, 8, [(5, 0, t, {})], canvas)                                     # leaves the canvas
    torch.cuda.synchronize()
    assert bool((canvas == FILL).all())                                           # nothing was launched


# ------------------------------------------------------------------------------------------------ from the renderer
def test_the_eval_render_packed_in_one_call(luts):
    """`step.render_scene_graph_eval` on a small scene graph with both layers on screen and a sky image: all of its
    outputs and a uint8 ground truth in one call; each view is the oracle applied to that output."""
    from sgn_rast import frames, ops, scenes, step
    W, H, FOCAL = 96, 64, 80.0
    cam = scenes.make_camera(W, H, FOCAL)
    models, poses, idft = scenes.make_scene_graph(4000, cam, n_objects=2, object_frac=0.2, fourier_dim=5, seed=3,
                                                  z_range=(1.5, 9.0), object_depth=(3.0, 7.0), object_extent=0.4)
    sky = torch.rand(H, W, 3, generator=torch.Generator().manual_seed(2)).to(DEV)
    models = [{k: v.to(DEV) for k, v in m.items()} for m in models]
    ops.clear_binning_cache()
    out = step.render_scene_graph_eval(models, poses.to(DEV), idft.to(DEV), scenes.make_camera(W, H, FOCAL, device=DEV),
                                       torch.tensor([0.1, 0.2, 0.3], device=DEV), sky=sky, fused=True)
    assert set(out) == {"rgb", "accumulation", "depth", "sky", "object_acc", "background_acc", "background_rgb",
                        "object_rgb"}
    assert float(out["object_acc"].max()) > 0.05 and float(out["background_acc"].max()) > 0.05   # both layers on screen
    out = dict(out, gt=torch.from_numpy(byte_values(H, W, 1)).to(DEV))
    rnd, gray = luts
    spec = {k: {} for k in out}
    spec["depth"] = dict(near=0.5, far=9.0, invert=True, lut=rnd)
    spec["accumulation"] = dict(near=0.0, far=1.0, invert=False, lut=gray)
    spec["object_acc"] = dict(near=0.0, far=1.0, invert=False, lut=rnd)
    spec["background_acc"] = dict(near=0.0, far=1.0, invert=True, lut=gray)
    order = ["gt"] + [k for k in out if k != "gt"]
    for arrange in ("column", "row"):
        canvas, views = frames.pack(out, to_panels(frames, spec, order), arrange=arrange)
        assert tuple(canvas.shape) == ((9 * H, W, 3) if arrange == "column" else (H, 9 * W, 3))
        for k in order:
            want = expected_panel(out[k].cpu().numpy(), spec[k])
            assert torch.equal(views[k].cpu(), torch.from_numpy(want)), (arrange, k)
        assert len(np.unique(views["depth"].cpu().numpy().reshape(-1, 3), axis=0)) > 16   # a picture, not a constant


# ------------------------------------------------------------------------------------------------ the ring
def _sink_frame(i, h, w):
    return {"rgb": torch.from_numpy(rgb_values(h, w, 30 + i)).to(DEV),
            "depth": torch.from_numpy(scalar_values(h, w, 0.5, 77.3, 40 + i, trailing=True)).to(DEV),
            "gt": torch.from_numpy(byte_values(h, w, 50 + i)).to(DEV)}


@pytest.mark.parametrize("slots,arrange,h,w", [(2, "column", 120, 256), (3, "row", 23, 37)])
def test_frame_sink_delivers_in_order_while_sources_are_overwritten(luts, slots, arrange, h, w):
    from sgn_rast import frames
    panels = [frames.Panel("rgb"), frames.Panel("depth", 0.5, 77.3, lut=luts[0][2]), frames.Panel("gt")]
    originals = [_sink_frame(i, h, w) for i in range(5)]
    want = [frames.pack(f, panels, arrange=arrange)[0].cpu().numpy() for f in originals]
    assert not np.array_equal(want[0], want[1])                                   # distinct content per frame
    got = []

    def on_frame(tag, canvas):
        assert isinstance(canvas, np.ndarray) and canvas.dtype == np.uint8
        got.append((tag, canvas.copy()))                                          # valid during the callback only

    with frames.FrameSink(panels, h, w, arrange=arrange, slots=slots, on_frame=on_frame) as sink:
        assert sink.drain() == [] and len(sink) == 0                              # nothing submitted: a no-op
        for i, f in enumerate(originals):
            work = {k: v.clone() for k, v in f.items()}
            sink.submit(work, tag=i)
            for v in work.values():
                v.fill_(7)                                                        # stream-ordered behind the pack
            assert len(sink) <= slots
            assert [t for t, _ in got] == list(range(len(got)))
        assert len(got) >= 5 - slots                                              # a full ring delivered the oldest
        sink.poll()
        assert sink.drain() == [] and len(sink) == 0
        assert sink.drain() == []
    assert [t for t, _ in got] == [0, 1, 2, 3, 4]
    for (tag, canvas), w_ in zip(got, want):
        assert canvas.shape == w_.shape and np.array_equal(canvas, w_), tag


def test_frame_sink_without_a_callback_returns_copies(luts):
    from sgn_rast import frames
    h, w = 23, 37
    panels = [frames.Panel("gt"), frames.Panel("depth", 0.5, 77.3, invert=True, lut="gray"), frames.Panel("rgb")]
    originals = [_sink_frame(i, h, w) for i in range(5)]
    sink = frames.FrameSink(panels, h, w, slots=2)
    sink.open()
    for i, f in enumerate(originals):
        sink.submit(f, tag=f"frame{i}")
    out = sink.drain()
    assert [t for t, _ in out] == [f"frame{i}" for i in range(5)] and sink.drain() == []
    for (tag, canvas), f in zip(out, originals):
        assert np.array_equal(canvas, frames.pack(f, panels)[0].cpu().numpy()), tag
    pinned = [m.numpy() for m in sink._host]
    assert all(not np.shares_memory(c, p) for _, c in out for p in pinned)        # copies, not views of the slots
    sink.submit(originals[0])                                                     # the sink stays usable after a drain
    (tag, canvas), = sink.close()
    assert tag is None and np.array_equal(canvas, out[0][1])
