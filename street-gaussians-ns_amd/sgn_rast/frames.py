"""Eval renders to the writers as bytes: a frame's outputs packed into one ``uint8`` canvas, moved behind the next render.

The reference's render script (``scripts/render.py:159-273``) runs every output of every frame through
``colormaps.apply_colormap`` / ``apply_depth_colormap`` (a three-channel output unchanged; a one-channel one clipped,
``(t * 255).long()``, a 256-row colour-table gather), moves the float32 result with ``.cpu().numpy()`` on the compute
stream and leaves the float -> ``uint8`` conversion to the image or video writer; the trainer's eval image
(``sgn_splatfacto.py:1134``) ends the same way.  Here one HIP kernel (``csrc/frame_pack.hip`` through
``sgn_frames_pack``) turns the outputs dict of :func:`sgn_rast.step.render_scene_graph_eval` — and the ``uint8`` ground
truth of a :class:`sgn_rast.feed.Batch` beside it — into those bytes on the device, and a small ring carries them to pinned
host memory while the next frame renders:

* :func:`byte_lut` / :func:`colormap` — a colour table as the 256 byte triples the reference's "gather a float table, let
  the writer quantise" produces.
* :class:`Panel` — which output, and for a one-channel output the planes, the inversion and the table.
* :func:`pack` — one launch: panels -> canvas ``uint8`` [CH,CW,3], a column of images or a side-by-side mosaic.
* :class:`FrameSink` — the outbound counterpart of :class:`sgn_rast.feed.ImageFeed`.

The arithmetic of the kernel is a contract (``include/sgn_rast.h``, ``tests/frames_oracle.py``): fp32, every operation
rounded on its own, so a canvas is bit for bit its restatement.  The float -> ``uint8`` rule, ``trunc(clip(x, 0, 1) * 255 +
0.5)``, is the writers' as recalled — unpinned: no writer library was at hand.  No CPU path.
"""
from __future__ import annotations

import collections
import collections.abc
import math
import numbers
import operator
import struct
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import torch

from . import _lib as L

MAX_DIM = 16384                    # sgn_frames_pack: 32-bit element indices
MAX_PANELS = L.FRAMES_MAX_PANELS
ARRANGEMENTS = ("column", "row")


# ------------------------------------------------------------------------------------------------ colour tables
def byte_lut(colors) -> torch.Tensor:
    """A float colour table [256,3] as ``uint8`` [256,3]: every entry through the writers' quantiser ``q(x) =
    trunc(clip(x, 0, 1) * 255 + 0.5)`` in float32 (NaN -> 0).  The reference gathers the float table per pixel and lets
    the writer quantise the gathered floats; quantising the 256 rows once gives the same bytes."""
    try:
        t = torch.as_tensor(colors, dtype=torch.float32).detach().cpu()
    except (TypeError, ValueError, RuntimeError):
        raise TypeError(f"colors must be a float table [256,3], got {type(colors).__name__}") from None
    if tuple(t.shape) != (256, 3):
        raise ValueError(f"colors must be [256,3], got {tuple(t.shape)}")
    one, zero = torch.ones((), dtype=torch.float32), torch.zeros((), dtype=torch.float32)
    c = torch.where(t > 0, torch.where(t < 1, t, one), zero)
    return (c * 255.0 + 0.5).to(torch.uint8)       # float32 multiply, float32 add, truncation


_tables: Dict[str, torch.Tensor] = {}              # name -> uint8 [256,3] on the host
_device_tables: Dict[Tuple[str, torch.device], torch.Tensor] = {}


def _table(name: str) -> torch.Tensor:
    """The host copy of a named table; raises before any device work."""
    if not isinstance(name, str):
        raise TypeError(f"a colour map is named by a str, got {type(name).__name__}")
    name = "turbo" if name == "default" else name          # nerfstudio's apply_float_colormap
    t = _tables.get(name)
    if t is not None:
        return t
    if name == "gray":
        t = byte_lut(torch.arange(256, dtype=torch.float32).div(255.0)[:, None].repeat(1, 3))
    else:
        try:
            import matplotlib
        except ImportError:
            raise ImportError(f'the colour map "{name}" is looked up in matplotlib, which is not installed; "gray" is '
                              "built in, and Panel(lut=) also takes a uint8 [256,3] tensor") from None
        try:
            colors = matplotlib.colormaps[name].colors
        except (KeyError, AttributeError):
            raise ValueError(f'"{name}" is not a listed matplotlib colour map with a 256-row table') from None
        t = byte_lut(colors)
    _tables[name] = t
    return t


def colormap(name: str = "default", device="cuda") -> torch.Tensor:
    """The table ``name`` as ``uint8`` [256,3] on ``device``, cached per ``(name, device)``.  ``"gray"`` is built in (row
    ``i`` is ``i / 255`` in all three channels, hence byte ``i``); any other name is ``matplotlib.colormaps[name].colors``
    through :func:`byte_lut`, as nerfstudio looks it up, with ``"default"`` -> ``"turbo"``; matplotlib is imported on
    first use and an ``ImportError`` says so when it is absent.  No table is stored in this package."""
    host = _table(name)
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    key = ("turbo" if name == "default" else name, dev)
    t = _device_tables.get(key)
    if t is None:
        t = _device_tables[key] = host.to(dev)
    return t


# ------------------------------------------------------------------------------------------------ panels
def _f32(v: float) -> float:
    return struct.unpack("f", struct.pack("f", v))[0]


class Panel:
    """``Panel(name, near=0.0, far=1.0, invert=False, lut="default")`` — one output of the frame and how it is shown.

    ``name`` is a key of the outputs dict.  What the panel does follows from the tensor found there, by the rule of
    ``render.py``: float32 with a last dimension of 3 is shown as it is (``RGB``); float32 [h,w] or [h,w,1] goes through
    the colour table (``SCALAR``); ``uint8`` [h,w,3] is copied (``BYTES``: ``gt-rgb`` straight from a feed batch).

    For a ``SCALAR`` panel ``t = (x - near) / (far - near + 1e-10)``, clipped to [0, 1], NaN -> 0, ``1 - t`` if
    ``invert``, and the pixel is row ``trunc(t * 255)`` of ``lut`` — ``apply_depth_colormap`` with the render script's
    ``depth_near_plane`` / ``depth_far_plane``.  The defaults ``near=0, far=1`` are ``apply_colormap``'s path for
    accumulations.  The reference's ``near_plane=None`` (the image's own minimum / maximum) stays with the caller as
    ``near=float(depth.min())``: there is no reduction in the kernel.  ``lut``: a name for :func:`colormap` or a ``uint8``
    [256,3] tensor on the outputs' device.

    ``TypeError`` / ``ValueError`` here, before any device work: the planes must be finite, and the fp32 denominator
    ``(float)((double)far - (double)near + 1e-10)`` must be finite and non-zero."""

    __slots__ = ("name", "near", "far", "invert", "lut", "lo", "den")

    def __init__(self, name: str, near: float = 0.0, far: float = 1.0, invert: bool = False,
                 lut: Union[str, torch.Tensor] = "default"):
        if not isinstance(name, str):
            raise TypeError(f"name must be a str (a key of the outputs), got {type(name).__name__}")
        for what, v in (("near", near), ("far", far)):
            if isinstance(v, bool) or not isinstance(v, numbers.Real):
                raise TypeError(f"{what} must be a real number, got {type(v).__name__}")
            if not math.isfinite(v):
                raise ValueError(f"{what} must be finite, got {v}")
        if not isinstance(invert, (bool, int)) or invert not in (0, 1):
            raise TypeError(f"invert must be a bool, got {invert!r}")
        if isinstance(lut, torch.Tensor):
            if lut.dtype != torch.uint8:
                raise TypeError(f"lut must be a uint8 table (byte_lut makes one from floats), got {lut.dtype}")
            if tuple(lut.shape) != (256, 3):
                raise ValueError(f"lut must be [256,3], got {tuple(lut.shape)}")
        elif not isinstance(lut, str):
            raise TypeError(f"lut must be a colour map's name or a uint8 [256,3] tensor, got {type(lut).__name__}")
        near, far = float(near), float(far)
        try:
            lo, den = _f32(near), _f32(far - near + 1e-10)
        except OverflowError:
            raise ValueError(f"near={near}, far={far} do not fit fp32") from None
        if not (math.isfinite(lo) and math.isfinite(den)) or den == 0.0:
            raise ValueError(f"near={near}, far={far}: the fp32 denominator far - near + 1e-10 is {den}; it must be "
                             "finite and non-zero")
        self.name, self.near, self.far, self.invert, self.lut, self.lo, self.den = name, near, far, bool(invert), lut, lo, den

    def __repr__(self) -> str:
        lut = self.lut if isinstance(self.lut, str) else "<table>"
        return f"Panel({self.name!r}, near={self.near}, far={self.far}, invert={self.invert}, lut={lut!r})"


def _check_panels(panels) -> List[Panel]:
    if isinstance(panels, (Panel, str)) or not isinstance(panels, collections.abc.Sequence):
        raise TypeError(f"panels must be a sequence of Panel, got {type(panels).__name__}")
    panels = list(panels)
    for p in panels:
        if not isinstance(p, Panel):
            raise TypeError(f"panels must hold Panel objects, got {type(p).__name__}")
    if not 1 <= len(panels) <= MAX_PANELS:
        raise ValueError(f"one call packs 1..{MAX_PANELS} panels, got {len(panels)}")
    names = [p.name for p in panels]
    if len(set(names)) != len(names):
        raise ValueError(f"panel names must differ (they key the views), got {names}")
    return panels


def _canvas_size(n: int, h: int, w: int, arrange: str) -> Tuple[int, int]:
    if arrange not in ARRANGEMENTS:
        raise ValueError(f'arrange must be "column" or "row", got {arrange!r}')
    if not (1 <= h <= MAX_DIM and 1 <= w <= MAX_DIM):
        raise ValueError(f"panel sides must lie in 1..{MAX_DIM}, got {h} x {w}")
    ch, cw = (n * h, w) if arrange == "column" else (h, n * w)
    if ch > MAX_DIM or cw > MAX_DIM:
        raise ValueError(f"the canvas of {n} panels of {h} x {w} in a {arrange} is {ch} x {cw}; sides are limited to "
                         f"{MAX_DIM}")
    return ch, cw


def _check_outputs(outputs, panels: List[Panel], hw: Optional[Tuple[int, int]]):
    """Host-side validation of one frame against its panels: ``TypeError`` / ``ValueError``; returns
    ``(h, w, [(kind, contiguous tensor)])``."""
    if not isinstance(outputs, collections.abc.Mapping):
        raise TypeError(f"outputs must be a mapping of names to tensors, got {type(outputs).__name__}")
    items = []
    for p in panels:
        if p.name not in outputs:
            raise ValueError(f"outputs has no {p.name!r} (it has {sorted(map(str, outputs))})")
        t = outputs[p.name]
        if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.uint8):
            what = t.dtype if isinstance(t, torch.Tensor) else type(t).__name__
            raise TypeError(f"outputs[{p.name!r}] must be a float32 or uint8 tensor, got {what}")
        shape = tuple(t.shape)
        if t.dtype == torch.uint8:
            if t.dim() != 3 or shape[2] != 3:
                raise ValueError(f"outputs[{p.name!r}]: a uint8 panel must be [h,w,3], got {shape}")
            kind = L.PANEL_BYTES
        elif t.dim() == 3 and shape[2] == 3:
            kind = L.PANEL_RGB
        elif t.dim() == 2 or (t.dim() == 3 and shape[2] == 1):
            kind = L.PANEL_SCALAR
        else:
            raise ValueError(f"outputs[{p.name!r}]: a float32 panel must be [h,w,3], [h,w] or [h,w,1], got {shape}")
        if shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"outputs[{p.name!r}] is empty: {shape}")
        if hw is None:
            hw = shape[:2]
        elif shape[:2] != tuple(hw):
            raise ValueError(f"all panels of a frame share one size: outputs[{p.name!r}] is {shape[0]} x {shape[1]}, "
                             f"expected {hw[0]} x {hw[1]}")
        if kind == L.PANEL_SCALAR and isinstance(p.lut, str):
            _table(p.lut)                               # ImportError / ValueError now, not after the launch
        items.append((kind, t))
    return int(hw[0]), int(hw[1]), items


def _check_out(out, ch: int, cw: int) -> None:
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8:
        what = out.dtype if isinstance(out, torch.Tensor) else type(out).__name__
        raise TypeError(f"out must be a uint8 tensor, got {what}")
    if tuple(out.shape) != (ch, cw, 3) or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous [{ch},{cw},3] canvas, got {tuple(out.shape)}")


def _launch(panels: List[Panel], h: int, w: int, items, arrange: str, canvas: Optional[torch.Tensor], ch: int, cw: int):
    tensors = [t for _, t in items]
    luts = [p.lut if kind == L.PANEL_SCALAR and isinstance(p.lut, torch.Tensor) else None
            for p, (kind, _) in zip(panels, items)]
    dev = L.require_device(canvas, *tensors, *luts)
    if canvas is None:
        canvas = torch.empty(ch, cw, 3, dtype=torch.uint8, device=dev)
    table = (L.PanelDesc * len(panels))()
    keep = []                                           # contiguous copies live until the launch is enqueued
    views = {}
    for i, (p, (kind, t)) in enumerate(zip(panels, items)):
        src = t.detach().contiguous()
        keep.append(src)
        d = table[i]
        d.src, d.kind = src.data_ptr(), kind
        d.y0, d.x0 = (i * h, 0) if arrange == "column" else (0, i * w)
        d.lo, d.den, d.invert = 0.0, 1.0, 0
        if kind == L.PANEL_SCALAR:
            lut = (luts[i] if luts[i] is not None else colormap(p.lut, dev)).contiguous()
            keep.append(lut)
            d.lut, d.lo, d.den, d.invert = lut.data_ptr(), p.lo, p.den, int(p.invert)
        views[p.name] = canvas[d.y0:d.y0 + h, d.x0:d.x0 + w]
    L.check(L.load().sgn_frames_pack(h, w, len(panels), table, L.ptr(canvas), ch, cw, L.stream_ptr()),
            "sgn_frames_pack")
    return canvas, views


def pack(outputs: Mapping[str, torch.Tensor], panels: Sequence[Panel], arrange: str = "column",
         out: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Dict[str, torch.Tensor]]:
    """The panels of one frame as bytes, in one launch: ``(canvas, views)``.

    ``outputs``: a mapping of names to device tensors, all ``h x w`` (see :class:`Panel` for the three kinds);
    ``panels``: 1..16 of them, in canvas order.  ``arrange="column"`` stacks them into ``canvas`` ``uint8`` [n*h, w, 3] —
    ``views[name]`` is then a contiguous [h,w,3] image of its own — and ``"row"`` puts them side by side into [h, n*w, 3]
    (the trainer's ``combined_rgb``); ``views`` maps every panel's name to its [h,w,3] view of the canvas.  ``out``: a
    contiguous ``uint8`` canvas of that shape to write into instead of a fresh one.  Canvas sides are limited to 16384.

    Everything is validated on the host first (``TypeError`` for wrong types and dtypes, ``ValueError`` for shapes, a
    missing key, mismatched sizes, more than 16 panels, an unknown arrangement; a missing matplotlib is an
    ``ImportError``), before any device call; CPU tensors then fail the library's device check (``SgnRastError``): there
    is no CPU path.  The launch goes to the current stream and nothing synchronises the host; the arithmetic is the
    contract of ``sgn_frames_pack`` (``include/sgn_rast.h``)."""
    panels = _check_panels(panels)
    h, w, items = _check_outputs(outputs, panels, None)
    ch, cw = _canvas_size(len(panels), h, w, arrange)
    if out is not None:
        _check_out(out, ch, cw)
    return _launch(panels, h, w, items, arrange, out, ch, cw)


# ------------------------------------------------------------------------------------------------ the ring
class FrameSink:
    """``FrameSink(panels, height, width, arrange="column", slots=2, on_frame=None, device="cuda")`` — the outbound
    counterpart of :class:`sgn_rast.feed.ImageFeed`: frames leave as bytes, behind the next frame's render.

    The sink owns ``slots`` device canvases, ``slots`` pinned host canvases of the same shape, one side stream and
    events; the constructor validates and allocates nothing (:meth:`open`, or the first :meth:`submit`).  The loop::

        with FrameSink(panels, H, W, on_frame=lambda tag, canvas: writer.add_image(canvas)) as sink:
            for i, cam in enumerate(cameras):
                out = render_scene_graph_eval(...)
                sink.submit({**out, "gt": batch.image}, tag=i)

    ``submit(outputs, tag)`` takes the next slot ``k``: the current stream waits for the previous copy out of slot ``k``,
    :func:`pack` writes device canvas ``k`` on the current stream, the side stream waits for that and copies the canvas
    to pinned canvas ``k``.  Once ``submit`` returns, the pack is enqueued: the caller may overwrite the source tensors
    with work on the same stream (the next render).  **``submit`` does not synchronise the host while the ring has a
    free slot**; with all ``slots`` frames outstanding it first waits for the oldest frame's copy and delivers it.
    :meth:`poll` delivers the frames whose copies have completed, without waiting; :meth:`drain` waits for and delivers
    all of them; leaving the ``with`` block (``close()``) drains.

    **Delivery and slot lifetime — the contract.**  Frames are delivered in submission order, on the calling thread, as
    ``on_frame(tag, canvas)``; ``canvas`` is a numpy ``uint8`` [CH,CW,3] array that is a *view of the pinned slot*, not a
    copy: it is valid for the duration of the callback only — the slot is handed to a later ``submit`` after it returns —
    so encode it or copy it there (``canvas.copy()``, or a panel of it: rows ``i*h .. (i+1)*h`` of a column).  With
    ``on_frame=None`` the sink copies each delivered canvas itself and ``drain()`` returns the list of ``(tag, copy)``
    since the last ``drain()``.  Encoding (PNG, JPEG, video) stays with the caller.
    """

    def __init__(self, panels: Sequence[Panel], height: int, width: int, arrange: str = "column", slots: int = 2,
                 on_frame: Optional[Callable] = None, device="cuda"):
        self.panels = _check_panels(panels)
        try:
            if isinstance(height, bool) or isinstance(width, bool):
                raise TypeError
            self.height, self.width = operator.index(height), operator.index(width)
        except TypeError:
            raise TypeError(f"height and width must be ints, got {height!r}, {width!r}") from None
        self.canvas_shape = _canvas_size(len(self.panels), self.height, self.width, arrange) + (3,)
        if isinstance(slots, bool) or not isinstance(slots, int):
            raise TypeError(f"slots must be an int, got {type(slots).__name__}")
        if slots < 2:
            raise ValueError(f"slots must be >= 2 (one being copied out, one being packed), got {slots}")
        if on_frame is not None and not callable(on_frame):
            raise TypeError(f"on_frame must be callable or None, got {type(on_frame).__name__}")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {self.device}")
        self.arrange, self.slots, self.on_frame = arrange, slots, on_frame
        self._opened = False
        self._queue: collections.deque = collections.deque()       # (slot, tag) of the frames not yet delivered
        self._kept: list = []                                       # on_frame=None: (tag, copy) since the last drain()

    def open(self) -> None:
        """Allocate the device canvases, the pinned canvases, the side stream and the events.  The first ``submit`` does
        this if nobody has (after its argument checks); call it to pay for the pinning up front."""
        if self._opened:
            return
        self._side = torch.cuda.Stream(device=self.device)
        self._dev = [torch.empty(self.canvas_shape, dtype=torch.uint8, device=self.device) for _ in range(self.slots)]
        for mem in self._dev:
            mem.record_stream(self._side)
        self._host = [torch.empty(self.canvas_shape, dtype=torch.uint8, pin_memory=True) for _ in range(self.slots)]
        self._packed = [torch.cuda.Event() for _ in range(self.slots)]   # current stream -> side stream: canvas k is packed
        self._done = [torch.cuda.Event() for _ in range(self.slots)]     # side stream -> host / current stream: copy k landed
        self._used = [False] * self.slots
        self._next = 0
        self._opened = True

    def __len__(self) -> int:
        """Frames submitted and not yet delivered."""
        return len(self._queue)

    def _deliver(self) -> None:
        k, tag = self._queue.popleft()
        canvas = self._host[k].numpy()                  # a view of the pinned slot
        if self.on_frame is None:
            self._kept.append((tag, canvas.copy()))
        else:
            self.on_frame(tag, canvas)

    def submit(self, outputs: Mapping[str, torch.Tensor], tag=None) -> None:
        """Pack ``outputs`` and start its copy to the host; see the class.  Host-side errors come first, as in
        :func:`pack`, and every tensor must be ``height x width``."""
        h, w, items = _check_outputs(outputs, self.panels, (self.height, self.width))
        L.require_device(*[t for _, t in items])
        self.open()
        if len(self._queue) == self.slots:              # the ring is full: the only host wait
            self._done[self._queue[0][0]].synchronize()
            self._deliver()
        k, self._next = self._next, (self._next + 1) % self.slots
        cur = torch.cuda.current_stream(self.device)
        if self._used[k]:
            cur.wait_event(self._done[k])               # the previous copy out of device canvas k
        _launch(self.panels, h, w, items, self.arrange, self._dev[k], self.canvas_shape[0], self.canvas_shape[1])
        self._packed[k].record(cur)
        self._side.wait_event(self._packed[k])
        with torch.cuda.stream(self._side):
            self._host[k].copy_(self._dev[k], non_blocking=True)
            self._done[k].record(self._side)
        self._used[k] = True
        self._queue.append((k, tag))

    def poll(self) -> int:
        """Deliver every frame whose copy has completed, oldest first, without waiting; returns how many."""
        n = 0
        while self._queue and self._done[self._queue[0][0]].query():
            self._deliver()
            n += 1
        return n

    def drain(self) -> list:
        """Wait for and deliver every outstanding frame.  Returns the ``(tag, copy)`` list collected since the last
        ``drain()`` when ``on_frame`` is ``None`` (an empty list otherwise).  A sink with nothing outstanding: a no-op."""
        while self._queue:
            self._done[self._queue[0][0]].synchronize()
            self._deliver()
        kept, self._kept = self._kept, []
        return kept

    def close(self) -> list:
        return self.drain()

    def __enter__(self) -> "FrameSink":
        return self

    def __exit__(self, *exc) -> bool:
        self.close()
        return False
