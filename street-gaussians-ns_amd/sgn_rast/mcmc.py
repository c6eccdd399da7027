"""Fixed-budget MCMC refinement ("3D Gaussian Splatting as Markov Chain Monte Carlo", Kheradmand et al. 2024; gsplat's
``MCMCStrategy``): the Gaussian count is an INPUT (``cap_max``), not an outcome of thresholds.  Four parts: a hard cap;
dead Gaussians teleported onto live ones sampled by opacity, with the opacity / scale correction that keeps the rendered
image unchanged; growth of 5 % per refinement up to the cap; a small opacity-gated noise on the means at every step.
The reference has no counterpart and gsplat is not a dependency: every behaviour below is decided here from the
published algorithm, unpinned.

:class:`MCMCDensifier` stands where :class:`sgn_rast.densify.Densifier` stands (same parameter dictionary, same per-name
optimisers, same ``after_train`` / ``refinement_after`` protocol), with ``engine="torch"`` (plain torch on any device)
or ``engine="hip"`` (``csrc/mcmc.hip``; device tensors only, no fallback).  The sampling is integer and hashed, so the
two engines — and every data-parallel replica — take the same decisions bit for bit.

THE ARITHMETIC CONTRACT is the header comment of ``csrc/mcmc.hip``; the module-level functions here (:func:`weights`,
:func:`draw`, :func:`relocation_values`, :func:`hash_normals`, :func:`noise_displacement`) are its torch restatement and
the torch engine is built from them.

Out of scope: the scene graph (``SceneGraphDensifier``, per-sub-model caps); ``train_step_views``; the reference's
opacity reset (MCMC has none).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L
from .densify import PARAM_NAMES, _mix64, leaf_like, rebind

RELOCATE, GROW, NOISE = 1, 2, 3                 # the phases p of key_p
N_MAX_LIMIT = 51                                # rows of the binomial table
_ROLES = {"opacity_logits": 1, "log_scales": 2}  # roles of sgn_mcmc_apply; every other parameter is 0, a moment 3
_BINOM = [[float(math.comb(m, k)) for k in range(N_MAX_LIMIT)] for m in range(N_MAX_LIMIT)]      # exact in fp64
_INV_SQRT = [1.0 / math.sqrt(k + 1.0) for k in range(N_MAX_LIMIT)]


@dataclass
class MCMCConfig:
    """gsplat's ``MCMCStrategy`` knobs.  ``noise_lr`` multiplies the means' CURRENT learning rate; ``n_max`` clamps the
    ratio of the relocation formula (and sizes its binomial table: at most 51); ``opacity_reg`` / ``scale_reg`` weigh
    :meth:`MCMCDensifier.regularizer`."""
    warmup_length: int = 500
    refine_every: int = 100
    stop_at: int = 25000
    cap_max: int = 1_000_000
    growth: float = 1.05
    min_opacity: float = 0.005
    noise_lr: float = 5e5
    n_max: int = 51
    opacity_reg: float = 0.01
    scale_reg: float = 0.01

    @property
    def absgrad(self) -> bool:
        """Read-only False: ``step.train_step`` reads ``densifier.cfg.absgrad``; MCMC keeps no gradient statistic."""
        return False


def _wrap64(v: int) -> int:
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


def phase_key(seed: int, step: int, phase: int) -> int:
    """``key_p = mix64(seed * 1_000_003 + step + (p << 56))`` as a signed 64-bit Python int."""
    return int(_mix64(torch.tensor(_wrap64(seed * 1_000_003 + step + (phase << 56)), dtype=torch.int64)).item())


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def weights(opacity_logits: torch.Tensor, min_opacity: float, relocate: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(``w`` int64 [n], ``dead`` bool [n]) of the contract's "weights"."""
    o = 1.0 / (1.0 + torch.exp(-opacity_logits.detach().reshape(-1).double()))
    dead = o <= _f32(min_opacity)
    w = torch.where(o == o, torch.floor(o * 16777216.0 + 0.5), torch.zeros_like(o)).to(torch.int64)
    if relocate:
        w = torch.where(dead, torch.zeros_like(w), w)
    return w, dead


def draw(w: torch.Tensor, k: int, key: int, n_max: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(``src`` int64 [k], ``ratio`` int64 [k]) of the contract's "draws" and "ratios"; ``w.sum() > 0``."""
    prefix = torch.cumsum(w, 0) - w
    total = int(w.sum().item())
    j = torch.arange(k, dtype=torch.int64, device=w.device)
    h = _mix64(_mix64(j + 1) ^ key)
    t = ((h >> 1) & 0x7FFFFFFFFFFFFFFF) % total
    src = torch.searchsorted(prefix, t, right=True) - 1
    count = torch.bincount(src, minlength=w.shape[0])
    return src, torch.clamp(1 + count[src], max=int(n_max))


def relocation_values(opacity_logits: torch.Tensor, log_scales: torch.Tensor, src: torch.Tensor, ratio: torch.Tensor,
                      min_opacity: float) -> torch.Tensor:
    """float32 [k, 4]: the new logit and the three new log-scales of every draw (the contract's "values")."""
    l = opacity_logits.detach().reshape(-1)[src].double()
    o = 1.0 / (1.0 + torch.exp(-l))
    x = 1.0 - torch.pow(1.0 - o, 1.0 / ratio.double())
    n_top = int(ratio.max().item()) if ratio.numel() else 0
    powers = [x]
    for _ in range(1, n_top):
        powers.append(powers[-1] * x)
    S, zero = torch.zeros_like(x), torch.zeros_like(x)
    for i in range(1, n_top + 1):
        inner = torch.zeros_like(x)
        for k in range(i):
            inner = inner + ((-_BINOM[i - 1][k] if k & 1 else _BINOM[i - 1][k]) * powers[k]) * _INV_SQRT[k]
        S = S + torch.where(ratio >= i, inner, zero)
    xc = torch.clamp(x, min=_f32(min_opacity), max=1.0 - 2.0 ** -23)
    logit = torch.log(xc / (1.0 - xc))
    scales = log_scales.detach()[src].double() + torch.log(o / S)[:, None]
    return torch.cat([logit[:, None], scales], dim=1).to(torch.float32)


def hash_normals(rows: torch.Tensor, key: int) -> torch.Tensor:
    """THE DEFINITION of the noise deviates: float32 [len(rows), 3] for int64 row numbers ``rows`` and ``key_3``.
    ``b = mix64(mix64(row + 1) ^ key)``; ``u_m = ((mix64(b + m) >>> 11) + 0.5) / 2^53``, m = 1..4; two Box-Muller pairs
    in fp64, three deviates kept (two logarithms a row), rounded to fp32."""
    b = _mix64(_mix64(rows.to(torch.int64) + 1) ^ key)
    u = [(((_mix64(b + m) >> 11) & 0x1FFFFFFFFFFFFF).to(torch.float64) + 0.5) * 2.0 ** -53 for m in (1, 2, 3, 4)]
    r1, r2 = torch.sqrt(-2.0 * torch.log(u[0])), torch.sqrt(-2.0 * torch.log(u[2]))
    a1, a2 = (2.0 * math.pi) * u[1], (2.0 * math.pi) * u[3]
    return torch.stack([r1 * torch.cos(a1), r1 * torch.sin(a1), r2 * torch.cos(a2)], dim=-1).to(torch.float32)


def noise_displacement(z: torch.Tensor, log_scales: torch.Tensor, quats: torch.Tensor, opacity_logits: torch.Tensor,
                       scaler: float) -> torch.Tensor:
    """``Sigma ((z * g) * scaler)`` [n, 3] of the contract's "noise", in the dtype of the inputs."""
    from .ops import quat_to_rotmat
    logit = opacity_logits.detach().reshape(-1)
    sig = 1.0 / (1.0 + torch.exp(-logit))
    g = 1.0 / (1.0 + torch.exp(-100.0 * ((1.0 - sig) - 0.995)))
    q = quats.detach()
    M = quat_to_rotmat(q / q.norm(dim=-1, keepdim=True)) * torch.exp(log_scales.detach())[:, None, :]
    v = (z * g[:, None]) * scaler
    return torch.bmm(torch.bmm(M, M.transpose(1, 2)), v[..., None]).squeeze(-1)


class MCMCDensifier:
    """The MCMC strategy over the parameter dictionary of :mod:`sgn_rast.step` (``densify.PARAM_NAMES``) and one
    optimiser per parameter (``torch.optim.Adam`` or :class:`sgn_rast.optim.FusedAdam`, state present or not yet
    created).  Call :meth:`refinement_after` after the optimiser step, on EVERY rank, EVERY step: inside the window it
    relocates, then grows; on every call it then adds the noise.  Relocation and noise are in place (same parameter and
    moment tensor objects, version counters bumped); growth allocates every tensor once at its final size and rebinds
    it in its optimiser (``densify.rebind``).  ``last`` keeps the stages of the latest relocate / grow phase (``w``,
    ``dead``, ``src``, ``targets``, ``ratio``, ``values``) for inspection.

    Out of scope: the scene graph, ``train_step_views``, the reference's opacity reset (MCMC has none)."""

    def __init__(self, params: Dict[str, torch.Tensor], optimizers: Dict[str, torch.optim.Optimizer],
                 config: MCMCConfig = MCMCConfig(), seed: int = 0, engine: str = "torch"):
        assert set(params) == set(PARAM_NAMES) and set(optimizers) >= set(PARAM_NAMES)
        if engine not in ("torch", "hip"):
            raise ValueError(f"MCMCDensifier: unknown engine {engine!r} (expected 'torch' or 'hip')")
        if not 1 <= int(config.n_max) <= N_MAX_LIMIT:
            raise ValueError(f"MCMCConfig.n_max must be in [1, {N_MAX_LIMIT}], got {config.n_max}")
        if engine == "hip":
            L.require_device(*params.values())
        self.params, self.optimizers, self.cfg, self.seed, self.engine = params, optimizers, config, int(seed), engine
        self.record: Dict[str, float] = {}
        self.last: Dict[str, dict] = {}

    # -------------------------------------------------------------------------------------------------- protocol
    def after_train(self, step: int, xys_grad: Optional[torch.Tensor], radii: torch.Tensor, last_size,
                    absgrad: Optional[torch.Tensor] = None) -> None:
        """``Densifier.after_train``'s arguments; MCMC keeps no per-step statistics."""

    def regularizer(self) -> torch.Tensor:
        """``opacity_reg * mean(sigmoid(opacity_logits)) + scale_reg * mean(exp(log_scales))``; ``step.train_step`` adds
        it to the loss."""
        P, c = self.params, self.cfg
        return c.opacity_reg * torch.sigmoid(P["opacity_logits"]).mean() + c.scale_reg * torch.exp(P["log_scales"]).mean()

    @torch.no_grad()
    def refinement_after(self, step: int) -> bool:
        """Returns True exactly when the number of Gaussians changed."""
        c = self.cfg
        n_before = self.params["means"].shape[0]
        if c.warmup_length < step < c.stop_at and step % c.refine_every == 0:
            self.last = {}
            relocated = self._phase(step, RELOCATE)
            added = self._phase(step, GROW)
            self.record.update(relocated_count=relocated, added_count=added,
                               gaussian_count=self.params["means"].shape[0])
        self.inject_noise(step)
        return self.params["means"].shape[0] != n_before

    # ---------------------------------------------------------------------------------------------------- pieces
    def _moments(self, name: str):
        st = self.optimizers[name].state.get(self.params[name], {})
        return [st[k] for k in ("exp_avg", "exp_avg_sq")] if "exp_avg" in st else []

    def _grow_count(self, n: int) -> int:
        return max(0, min(int(self.cfg.cap_max), int(self.cfg.growth * n)) - n)

    def _phase(self, step: int, phase: int) -> int:
        """One relocate or grow phase; returns the number of draws applied."""
        n = self.params["means"].shape[0]
        if n == 0 or (phase == GROW and self._grow_count(n) == 0):
            return 0
        key = phase_key(self.seed, step, phase)
        run = self._phase_hip if self.engine == "hip" else self._phase_torch
        stage = run(n, phase, key)
        self.last["relocate" if phase == RELOCATE else "grow"] = stage
        return int(stage["src"].shape[0])

    def _empty_stage(self, w, dead, dev) -> dict:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return dict(w=w, dead=dead, src=e, targets=e, ratio=e, values=torch.empty(0, 4, device=dev))

    def _phase_torch(self, n: int, phase: int, key: int) -> dict:
        P, c = self.params, self.cfg
        dev = P["means"].device
        w, dead = weights(P["opacity_logits"], c.min_opacity, relocate=phase == RELOCATE)
        k = int(dead.sum().item()) if phase == RELOCATE else self._grow_count(n)
        if k == 0 or int(w.sum().item()) == 0:
            return self._empty_stage(w, dead, dev)
        src, ratio = draw(w, k, key, c.n_max)
        values = relocation_values(P["opacity_logits"], P["log_scales"], src, ratio, c.min_opacity)
        computed = {"opacity_logits": values[:, :1], "log_scales": values[:, 1:]}
        if phase == RELOCATE:
            targets = torch.nonzero(dead).reshape(-1)
            for name in PARAM_NAMES:
                p = P[name].detach()
                if name in computed:
                    p[targets] = computed[name].reshape((k,) + tuple(p.shape[1:]))
                    p[src] = computed[name].reshape((k,) + tuple(p.shape[1:]))
                else:
                    p[targets] = p[src]
                for m in self._moments(name):
                    m[src] = 0
        else:
            targets = torch.arange(n, n + k, dtype=torch.int64, device=dev)
            for name in PARAM_NAMES:
                old = P[name].detach()
                new = torch.empty((n + k,) + tuple(old.shape[1:]), dtype=old.dtype, device=dev)
                new[:n] = old
                if name in computed:
                    v = computed[name].reshape((k,) + tuple(old.shape[1:]))
                    new[src] = v
                    new[n:] = v
                else:
                    new[n:] = old[src]
                rebind(P, self.optimizers, name, leaf_like(P[name], new),
                       lambda t: torch.cat([t, t.new_zeros((k,) + tuple(t.shape[1:]))], dim=0))
        return dict(w=w, dead=dead, src=src, targets=targets, ratio=ratio, values=values)

    def _phase_hip(self, n: int, phase: int, key: int) -> dict:
        """weights -> scan -> ONE host read (the totals) -> draw -> relocation -> apply."""
        P, c, lib = self.params, self.cfg, L.load()
        old = {name: P[name].detach() for name in PARAM_NAMES}
        dev = L.require_device(*old.values())
        for name, t in old.items():
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"MCMCDensifier(engine='hip') needs contiguous fp32 parameters ({name})")
        i32 = dict(dtype=torch.int32, device=dev)
        ws = L.workspace(lib.sgn_mcmc_workspace_bytes(n), dev)
        w, dead = torch.empty(n, **i32), torch.empty(n, dtype=torch.uint8, device=dev)
        prefix, dead_rows = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, **i32)
        totals_dev = torch.empty(2, dtype=torch.int64, device=dev)
        s = L.stream_ptr()
        L.check(lib.sgn_mcmc_weights(n, L.ptr(old["opacity_logits"]), c.min_opacity, int(phase == RELOCATE), L.ptr(w),
                                     L.ptr(dead), L.ptr(ws), ws.numel(), s), "sgn_mcmc_weights")
        L.check(lib.sgn_mcmc_scan(n, L.ptr(w), L.ptr(dead), L.ptr(prefix), L.ptr(dead_rows), L.ptr(ws), ws.numel(),
                                  L.ptr(totals_dev), s), "sgn_mcmc_scan")
        if getattr(self, "_totals_host", None) is None:
            self._totals_host = torch.empty(2, dtype=torch.int64, pin_memory=True)
        self._totals_host.copy_(totals_dev, non_blocking=True)
        torch.cuda.current_stream(dev).synchronize()                 # the one host read of the phase
        n_dead, total = self._totals_host.tolist()
        k = n_dead if phase == RELOCATE else self._grow_count(n)
        if k == 0 or total == 0:
            return self._empty_stage(w, dead.bool(), dev)
        src, ratio = torch.empty(k, **i32), torch.empty(k, **i32)
        values = torch.empty(k, 4, dtype=torch.float32, device=dev)
        L.check(lib.sgn_mcmc_draw(n, k, key, int(c.n_max), L.ptr(prefix), L.ptr(src), L.ptr(ratio), L.ptr(ws),
                                  ws.numel(), s), "sgn_mcmc_draw")
        L.check(lib.sgn_mcmc_relocation(n, k, L.ptr(old["opacity_logits"]), L.ptr(old["log_scales"]), c.min_opacity,
                                        L.ptr(src), L.ptr(ratio), L.ptr(values), s), "sgn_mcmc_relocation")
        new, moments, rows = {}, {}, []                   # rows: (input, output, floats per row, role)
        for name in PARAM_NAMES:
            t = old[name]
            rf = int(t[0].numel())
            ms = [m.detach() for m in self._moments(name)]
            L.require_device(*ms)
            if any(m.dtype != torch.float32 or not m.is_contiguous() or m.shape != t.shape for m in ms):
                raise ValueError(f"MCMCDensifier(engine='hip') needs contiguous fp32 Adam moments ({name})")
            if phase == RELOCATE:
                new[name], moments[name] = t, ms
            else:
                new[name] = torch.empty((n + k,) + tuple(t.shape[1:]), dtype=torch.float32, device=dev)
                moments[name] = [torch.empty_like(new[name]) for _ in ms]
            if rf > 0:                                    # (SH degree 0: features_rest has no columns)
                rows.append((t, new[name], rf, _ROLES.get(name, 0)))
                rows += [(m, o, rf, 3) for m, o in zip(ms, moments[name])]
        cnt = len(rows)
        L.check(lib.sgn_mcmc_apply(
            0 if phase == RELOCATE else 1, n, k, L.ptr(src), L.ptr(dead_rows), L.ptr(values), cnt,
            (C.c_void_p * cnt)(*[r[0].data_ptr() for r in rows]), (C.c_void_p * cnt)(*[r[1].data_ptr() for r in rows]),
            (C.c_int32 * cnt)(*[r[2] for r in rows]), (C.c_int32 * cnt)(*[r[3] for r in rows]), L.ptr(ws), ws.numel(),
            s), "sgn_mcmc_apply")
        if phase == RELOCATE:
            # the kernel wrote through raw pointers: the binning and SH caches key on the version (optim._launch)
            torch.autograd.graph.increment_version([r[1] for r in rows])
            targets = dead_rows[:k]
        else:
            for name in PARAM_NAMES:                      # the optimiser surgery, once per parameter
                it = iter(moments[name])
                rebind(P, self.optimizers, name, leaf_like(P[name], new[name]), lambda t, it=it: next(it))
            targets = torch.arange(n, n + k, **i32)
        return dict(w=w, dead=dead.bool(), src=src, targets=targets, ratio=ratio, values=values)

    @torch.no_grad()
    def inject_noise(self, step: int, z_out: Optional[torch.Tensor] = None) -> None:
        """``means += Sigma ((z * g) * scaler)`` with ``scaler = lr(means) * noise_lr``, in place.  ``z_out`` [n,3]
        float32 (tests) receives the deviates."""
        P, c = self.params, self.cfg
        means = P["means"].detach()
        n = means.shape[0]
        if n == 0:
            return
        scaler = self.optimizers["means"].param_groups[0]["lr"] * c.noise_lr
        key = phase_key(self.seed, step, NOISE)
        if self.engine == "hip":
            ts = [means] + [P[k].detach() for k in ("log_scales", "quats", "opacity_logits")]
            dev = L.require_device(*ts, z_out)
            if any(t.dtype != torch.float32 or not t.is_contiguous() for t in ts + ([] if z_out is None else [z_out])):
                raise ValueError("MCMCDensifier(engine='hip') needs contiguous fp32 parameters")
            if z_out is not None and tuple(z_out.shape) != (n, 3):
                raise ValueError(f"z_out must be [{n}, 3]")
            L.check(L.load().sgn_mcmc_noise(n, key, scaler, *[L.ptr(t) for t in ts], L.ptr(z_out), L.stream_ptr()),
                    "sgn_mcmc_noise")
            torch.autograd.graph.increment_version([means])
            return
        z = hash_normals(torch.arange(n, dtype=torch.int64, device=means.device), key)
        if z_out is not None:
            z_out.copy_(z)
        means.add_(noise_displacement(z, P["log_scales"], P["quats"], P["opacity_logits"], scaler))
