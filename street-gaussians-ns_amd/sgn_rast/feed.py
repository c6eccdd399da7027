"""Ground-truth feed of the training loop: the data set as bytes, the next step's batch on the device ahead of the step.

The reference's ``FullImageDatamanager.next_train`` (``data/sgn_datamanager.py:277-293``) deep-copies a cached float32
image and moves it with ``.to(self.device)`` on the compute stream, in front of the step, every step: 29.5 MB at
1920x1280 with nothing to overlap it, the semantic map as int64 beside it, and the whole cache as float32 in host memory.
:class:`ImageFeed` keeps the cache as ``uint8`` (what the files hold; a quarter of the host memory and of the PCIe
traffic) and hands the loss the bytes themselves: ``sgn_rast.loss`` reads a ``uint8`` ground truth in its kernels
(``sgn_l1_ssim_gt8_fwd/bwd``), so nothing is converted on the way.

* ``cache="pinned"`` — the items live in pinned host memory; ``slots`` device slots, one side stream and events carry
  one step's items across while the previous step computes.
* ``cache="device"`` — everything resident on the device as ``uint8`` (the reference's ``cache_images="gpu"``);
  :meth:`ImageFeed.get` returns views and :meth:`ImageFeed.prefetch` does nothing.

Plain torch: pinned tensors, streams, events.  Neither call synchronises the host.
"""
from __future__ import annotations

import operator
from typing import List, NamedTuple, Optional, Sequence, Tuple, Union

import torch

from .loss import check_mask

ALIGN = 256      # every item, and every part of one, starts on a 256-byte boundary of its slot


class Batch(NamedTuple):
    """One item on the device: ``image`` uint8 [H,W,3]; ``mask`` in the dtype and shape it was given (``bool`` or
    ``uint8``, [H,W] or [H,W,1]) or ``None``; ``semantic`` uint8 in the shape it was given, or ``None``."""
    image: torch.Tensor
    mask: Optional[torch.Tensor]
    semantic: Optional[torch.Tensor]


def _up(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


class _Item(NamedTuple):
    """Where the parts of one item lie in its blob (byte offsets; -1: absent) and how to view them."""
    nbytes: int
    hw: Tuple[int, int]
    mask_off: int
    mask_shape: Optional[Tuple[int, ...]]
    mask_bool: bool
    sem_off: int
    sem_shape: Optional[Tuple[int, ...]]


def _check_image(i: int, img) -> Tuple[int, int]:
    if not isinstance(img, torch.Tensor) or img.dtype != torch.uint8:
        what = img.dtype if isinstance(img, torch.Tensor) else type(img).__name__
        raise TypeError(f"images[{i}] must be a uint8 tensor (the bytes of the image file), got {what}")
    if img.dim() != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"images[{i}] must be [H,W,3], got {tuple(img.shape)}")
    if img.device.type != "cpu":
        raise ValueError(f"images[{i}] must be a CPU tensor, got one on {img.device}")
    return int(img.shape[0]), int(img.shape[1])


def _check_semantic(i: int, sem, h: int, w: int) -> None:
    if not isinstance(sem, torch.Tensor) or sem.dtype == torch.bool or sem.is_floating_point() or sem.is_complex():
        what = sem.dtype if isinstance(sem, torch.Tensor) else type(sem).__name__
        raise TypeError(f"semantics[{i}] must be an integer tensor of class ids, got {what}")
    if tuple(sem.shape) not in ((h, w), (h, w, 1)):
        raise ValueError(f"semantics[{i}] must be [{h},{w}] or [{h},{w},1] like its image, got {tuple(sem.shape)}")
    if sem.device.type != "cpu":
        raise ValueError(f"semantics[{i}] must be a CPU tensor, got one on {sem.device}")
    lo, hi = int(sem.min()), int(sem.max())
    if lo < 0 or hi > 255:
        raise ValueError(f"semantics[{i}] is stored as uint8: values must lie in 0..255, got {lo}..{hi}")


def _per_item(name: str, seq, n: int) -> list:
    if seq is None:
        return [None] * n
    seq = list(seq)
    if len(seq) != n:
        raise ValueError(f"{name} must have one entry per image ({n}), got {len(seq)}")
    return seq


class ImageFeed:
    """``ImageFeed(images, masks=None, semantics=None, device="cuda", cache="pinned" | "device", slots=2, batch=1)``

    ``images``: a sequence of ``uint8`` [H_i,W_i,3] CPU tensors; the sizes may differ from item to item (side cameras).
    ``masks``: per item ``None`` or a ``bool`` / ``uint8`` [H_i,W_i] or [H_i,W_i,1] tensor (non-zero = keep).
    ``semantics``: per item an integer tensor [H_i,W_i] or [H_i,W_i,1] with values 0..255, stored as ``uint8``
    (``loss.accumulation_losses`` takes ``uint8``).  Everything is validated on the host, ``TypeError`` / ``ValueError``,
    before any device work; the constructor itself allocates nothing (:meth:`open`).

    ``prefetch(i)`` (or a sequence of at most ``batch`` indices: one step's items) enqueues the host-to-device copies
    into the next slot on the feed's side stream.  ``get(i)`` returns :class:`Batch` (a list of them for a sequence):
    device tensors that are views into the slot; it makes the *current* stream wait for the copy's event.  A ``get`` of
    something that was not prefetched, or of something else than was prefetched, issues the copy itself.  The loop:

        feed.prefetch(order[0])
        for s in range(steps):
            b = feed.get(order[s])
            feed.prefetch(order[s + 1])
            train_step(..., gt=b.image, mask=b.mask)

    **Slot lifetime — the contract.**  What ``get`` returns is a view of a slot, not a copy.  A slot is overwritten only
    by a ``prefetch`` (or the copy of an un-prefetched ``get``) issued after a later ``get``: with ``slots=2`` the tensors
    of ``get`` number *s* stay intact until the ``prefetch`` that follows ``get`` number *s + 1*.  Before that copy starts,
    the side stream waits for an event recorded on the current stream at that ``prefetch`` call, so everything
    enqueued until then finishes first — the backward that reads the ground truth included.  Hence: enqueue all work
    that reads a batch, on the stream that is current when ``prefetch`` is called, before the ``prefetch`` after the
    next ``get``; keep a tensor longer only as a ``clone()``.  A ``prefetch`` that follows another without a ``get``
    between them replaces it in the same slot.  More ``slots`` extend the lifetime by one ``get`` each.

    ``cache="device"``: the items are resident on the device as ``uint8``; ``get`` returns views that stay valid for
    the feed's life and ``prefetch`` only checks its indices.
    """

    def __init__(self, images: Sequence[torch.Tensor], masks=None, semantics=None, device="cuda", cache: str = "pinned",
                 slots: int = 2, batch: int = 1):
        if cache not in ("pinned", "device"):
            raise ValueError(f'cache must be "pinned" or "device", got {cache!r}')
        if not isinstance(slots, int) or slots < 2:
            raise ValueError(f"slots must be an integer >= 2 (one being read, one being filled), got {slots!r}")
        if not isinstance(batch, int) or batch < 1:
            raise ValueError(f"batch must be an integer >= 1, got {batch!r}")
        images = list(images)
        if not images:
            raise ValueError("images is empty")
        n = len(images)
        masks, semantics = _per_item("masks", masks, n), _per_item("semantics", semantics, n)
        self._items: List[_Item] = []
        for i, img in enumerate(images):
            h, w = _check_image(i, img)
            off = _up(h * w * 3)
            mask_off, mask_shape, mask_bool, sem_off, sem_shape = -1, None, False, -1, None
            if masks[i] is not None:
                check_mask(masks[i], h, w)
                if masks[i].device.type != "cpu":
                    raise ValueError(f"masks[{i}] must be a CPU tensor, got one on {masks[i].device}")
                mask_off, mask_shape, mask_bool = off, tuple(masks[i].shape), masks[i].dtype == torch.bool
                off += _up(h * w)
            if semantics[i] is not None:
                _check_semantic(i, semantics[i], h, w)
                sem_off, sem_shape = off, tuple(semantics[i].shape)
                off += _up(h * w)
            self._items.append(_Item(off, (h, w), mask_off, mask_shape, mask_bool, sem_off, sem_shape))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError(f"device must be a GPU, got {self.device}")
        self.cache, self.slots, self.batch = cache, slots, batch
        self._source = (images, masks, semantics)                    # until open() has packed them
        self._blobs: List[torch.Tensor] = []

    def open(self) -> None:
        """Allocate the storage and pack the items into it: pinned host memory and the device slots, or the resident
        device copies.  The first ``prefetch`` or ``get`` does this if nobody has (after checking its indices, so every
        argument error of the feed comes before any device work); call it to pay for the pinning up front."""
        if self._source is None:
            return
        (images, masks, semantics), self._source = self._source, None
        pinned, slots, batch = self.cache == "pinned", self.slots, self.batch
        for it, img, mask, sem in zip(self._items, images, masks, semantics):
            h, w = it.hw
            blob = torch.zeros(it.nbytes, dtype=torch.uint8, pin_memory=pinned)
            blob[:h * w * 3].copy_(img.reshape(-1))
            if mask is not None:
                m = mask.contiguous()
                blob[it.mask_off:it.mask_off + h * w].copy_((m.view(torch.uint8) if it.mask_bool else m).reshape(-1))
            if sem is not None:
                blob[it.sem_off:it.sem_off + h * w].copy_(sem.reshape(-1).to(torch.uint8))
            self._blobs.append(blob.to(self.device) if not pinned else blob)
        if not pinned:
            return
        self._stride = max(it.nbytes for it in self._items)          # already a multiple of ALIGN
        self._side = torch.cuda.Stream(device=self.device)
        self._slot_mem = [torch.empty(batch * self._stride, dtype=torch.uint8, device=self.device) for _ in range(slots)]
        for mem in self._slot_mem:
            mem.record_stream(self._side)
        self._free = [torch.cuda.Event() for _ in range(slots)]      # consumer stream -> side stream: the slot may be written
        self._ready = [torch.cuda.Event() for _ in range(slots)]     # side stream -> consumer stream: the copy has landed
        self._held: List[Optional[Tuple[int, ...]]] = [None] * slots  # the indices each slot holds (or is being filled with)
        self._next = 0                                               # the slot the next batch goes to
        self._pending: Optional[int] = None                          # the slot of a prefetch no get has taken yet

    def __len__(self) -> int:
        return len(self._items)

    def _indices(self, idx) -> Tuple[Tuple[int, ...], bool]:
        try:
            ids, single = (operator.index(idx),), True
        except TypeError:
            ids, single = tuple(operator.index(i) for i in idx), False
        if not ids or len(ids) > self.batch:
            raise ValueError(f"a step has 1..{self.batch} items (batch={self.batch}), got {len(ids)}")
        for i in ids:
            if not 0 <= i < len(self._items):
                raise IndexError(f"index {i} is outside the feed's {len(self._items)} items")
        self.open()
        return ids, single

    def _views(self, it: _Item, mem: torch.Tensor) -> Batch:
        h, w = it.hw
        image = mem[:h * w * 3].view(h, w, 3)
        mask = semantic = None
        if it.mask_off >= 0:
            mask = mem[it.mask_off:it.mask_off + h * w].view(it.mask_shape)
            if it.mask_bool:
                mask = mask.view(torch.bool)
        if it.sem_off >= 0:
            semantic = mem[it.sem_off:it.sem_off + h * w].view(it.sem_shape)
        return Batch(image, mask, semantic)

    def _enqueue(self, ids: Tuple[int, ...]) -> int:
        """The copies of one step's items into a slot nobody holds a live view of; returns the slot."""
        if self._pending is not None:
            k = self._pending                    # never handed out: the side stream is in order, the new copy follows the old
        else:
            k, self._next = self._next, (self._next + 1) % self.slots
        self._free[k].record(torch.cuda.current_stream(self.device))
        self._side.wait_event(self._free[k])     # everything enqueued so far, the readers of this slot among it, ends first
        with torch.cuda.stream(self._side):
            for j, i in enumerate(ids):
                n = self._items[i].nbytes
                self._slot_mem[k][j * self._stride:j * self._stride + n].copy_(self._blobs[i], non_blocking=True)
            self._ready[k].record(self._side)
        self._held[k], self._pending = ids, k
        return k

    def prefetch(self, idx: Union[int, Sequence[int]]) -> None:
        """Start the copies of the items the next ``get`` will ask for.  No host synchronisation."""
        ids, _ = self._indices(idx)
        if self.cache == "pinned":
            self._enqueue(ids)

    def get(self, idx: Union[int, Sequence[int]]):
        """:class:`Batch` of item ``idx``, or the list of them for a sequence of indices; see the class for how long
        the tensors stay valid.  No host synchronisation."""
        ids, single = self._indices(idx)
        if self.cache == "device":
            out = [self._views(self._items[i], self._blobs[i]) for i in ids]
            return out[0] if single else out
        k = self._pending
        if k is None or self._held[k] != ids:
            k = self._enqueue(ids)
        self._pending = None
        torch.cuda.current_stream(self.device).wait_event(self._ready[k])
        out = [self._views(self._items[i], self._slot_mem[k][j * self._stride:(j + 1) * self._stride])
               for j, i in enumerate(ids)]
        return out[0] if single else out
