"""Independent oracle of the MCMC refinement's arithmetic contract (csrc/mcmc.hip's header comment), written from the
formulas with Python ints, numpy fp64 and ``decimal``.  It imports nothing from ``sgn_rast.mcmc``.

The yardstick every comparison asserts first (:func:`violations`): in fp64 no ``o * 2^24`` lies within 1e-6 of a
half-integer and no ``o`` within a relative 1e-9 of ``min_opacity`` — :func:`make_world` resamples the few rows that
do.  With that margin the integer stages of any correct engine equal the oracle's exactly; no row is excused."""
import decimal
import math

import numpy as np

M64 = (1 << 64) - 1
NAMES = ("means", "log_scales", "quats", "features_dc", "features_rest", "opacity_logits")
SHAPES = dict(means=(3,), log_scales=(3,), quats=(4,), features_dc=(1, 3), features_rest=(3, 3), opacity_logits=(1,))


def mix64(x: int) -> int:
    x = (x * 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def mix64_np(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = x.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def phase_key(seed: int, step: int, phase: int) -> int:
    """Unsigned 64-bit."""
    return mix64((seed * 1_000_003 + step + (phase << 56)) & M64)


def signed(v: int) -> int:
    return v - (1 << 64) if v >= (1 << 63) else v


def f32(v: float) -> float:
    return float(np.float32(v))


def opacity64(logits) -> np.ndarray:
    return 1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float32).reshape(-1).astype(np.float64)))


def violations(logits, min_opacity: float) -> np.ndarray:
    """Rows on which an engine's fp64 could legitimately round the other way."""
    o = opacity64(logits)
    scaled = o * 16777216.0
    near_half = np.abs((scaled - np.floor(scaled)) - 0.5) < 1e-6
    m = f32(min_opacity)
    return near_half | (np.abs(o - m) < 1e-9 * m)


def weights(logits, min_opacity: float, relocate: bool):
    """(w int64 [n], dead bool [n])."""
    o = opacity64(logits)
    dead = o <= f32(min_opacity)
    w = np.floor(o * 16777216.0 + 0.5).astype(np.int64)
    if relocate:
        w = np.where(dead, 0, w)
    return w, dead


def draw(w: np.ndarray, k: int, key: int, n_max: int):
    """(src int64 [k], ratio int64 [k]); Python ints for the modulo."""
    prefix = np.cumsum(w) - w
    total = int(w.sum())
    h = mix64_np(mix64_np(np.arange(1, k + 1, dtype=np.uint64)) ^ np.uint64(key))
    t = np.array([(int(v) >> 1) % total for v in h], dtype=np.int64)
    src = np.searchsorted(prefix, t, side="right") - 1
    assert np.all((prefix[src] <= t) & (t < prefix[src] + w[src]))
    count = np.bincount(src, minlength=w.shape[0])
    return src.astype(np.int64), np.minimum(n_max, 1 + count[src]).astype(np.int64)


def relocation_values64(logits, log_scales, src, ratio, min_opacity: float) -> np.ndarray:
    """fp64 [k, 4]: new logit and new log-scales, the literal double sum, NOT yet rounded to fp32.  (Draws that share a
    source share its ratio: evaluated once per distinct source.)"""
    src, ratio = np.asarray(src, dtype=np.int64), np.asarray(ratio, dtype=np.int64)
    uniq, first, inverse = np.unique(src, return_index=True, return_inverse=True)
    if uniq.shape[0] < src.shape[0]:
        assert np.array_equal(ratio[first][inverse], ratio)
        return relocation_values64(logits, log_scales, uniq, ratio[first], min_opacity)[inverse]
    o = opacity64(logits)[src]
    N = ratio
    x = 1.0 - np.power(1.0 - o, 1.0 / N)
    S = np.zeros_like(x)
    for i in range(1, int(N.max()) + 1 if N.size else 1):
        inner = np.zeros_like(x)
        for k in range(i):
            inner += math.comb(i - 1, k) * (-1.0) ** k * x ** (k + 1) / math.sqrt(k + 1)
        S += np.where(N >= i, inner, 0.0)
    xc = np.clip(x, f32(min_opacity), 1.0 - 2.0 ** -23)
    ls = np.asarray(log_scales, dtype=np.float32).astype(np.float64)[src]
    return np.concatenate([np.log(xc / (1.0 - xc))[:, None], ls + np.log(o / S)[:, None]], axis=1)


def relocation_decimal(logit: float, n: int, digits: int = 60):
    """(x, o / S) of one draw in ``digits``-digit decimal arithmetic from the fp32 logit."""
    with decimal.localcontext() as ctx:
        ctx.prec = digits
        D = decimal.Decimal
        o = 1 / (1 + (-D(float(np.float32(logit)))).exp())
        x = 1 - ((1 - o).ln() / n).exp()
        S = D(0)
        for i in range(1, n + 1):
            for k in range(i):
                S += math.comb(i - 1, k) * (-1) ** k * x ** (k + 1) / D(k + 1).sqrt()
        return x, o / S


def normals64(rows: np.ndarray, key: int) -> np.ndarray:
    """fp64 [n, 3] Box-Muller deviates of the noise phase."""
    b = mix64_np(mix64_np(rows.astype(np.uint64) + np.uint64(1)) ^ np.uint64(key))
    with np.errstate(over="ignore"):
        u = [((mix64_np(b + np.uint64(m)) >> np.uint64(11)).astype(np.float64) + 0.5) / 9007199254740992.0
             for m in (1, 2, 3, 4)]
    r1, r2 = np.sqrt(-2.0 * np.log(u[0])), np.sqrt(-2.0 * np.log(u[2]))
    return np.stack([r1 * np.cos(2.0 * np.pi * u[1]), r1 * np.sin(2.0 * np.pi * u[1]),
                     r2 * np.cos(2.0 * np.pi * u[3])], axis=-1)


def rotmat64(quats) -> np.ndarray:
    q = np.asarray(quats, dtype=np.float64)
    w, x, y, z = (q / np.linalg.norm(q, axis=-1, keepdims=True)).T
    return np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=-1).reshape(-1, 3, 3)


def noise64(z32, log_scales, quats, logits, scaler: float):
    """fp64 evaluation of the displacement from the fp32 deviates and parameters: (d [n,3], normaliser [n], g [n]) with
    normaliser = |Sigma|_F * |z| * g * scaler."""
    z = np.asarray(z32, dtype=np.float64)
    g = 1.0 / (1.0 + np.exp(-100.0 * ((1.0 - opacity64(logits)) - 0.995)))
    R = rotmat64(quats)
    s2 = np.exp(np.asarray(log_scales, dtype=np.float64)) ** 2
    Sigma = np.einsum("nij,nj,nkj->nik", R, s2, R)
    sc = f32(scaler)
    d = np.einsum("nij,nj->ni", Sigma, z * g[:, None] * sc)
    return d, np.linalg.norm(Sigma, axis=(1, 2)) * np.linalg.norm(z, axis=1) * g * sc, g


def ulp32(v) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(v, dtype=np.float32))).astype(np.float64)


def within_ulp(got32, want64, floor: float) -> np.ndarray:
    """|got - fl32(want)| <= max(1 ulp of fl32(want), floor), elementwise."""
    want32 = np.asarray(want64, dtype=np.float64).astype(np.float32)
    diff = np.abs(np.asarray(got32, dtype=np.float64) - want32.astype(np.float64))
    return diff <= np.maximum(ulp32(want32), floor)


# ------------------------------------------------------------------------------------------------------ worlds
def _logits(rng, n: int, dead: np.ndarray) -> np.ndarray:
    live = rng.uniform(-4.0, 6.0, n)            # sigmoid(-4) = 0.018 > min_opacity = 0.005 = sigmoid(-5.29)
    gone = rng.uniform(-9.0, -5.6, n)
    return np.where(dead, gone, live).astype(np.float32)


def make_world(n: int, kind, seed: int = 0, min_opacity: float = 0.005):
    """The 18 tensors (6 parameters + their exp_avg / exp_avg_sq) as float32 numpy arrays, name -> [n, ...], moments as
    ``name + '.exp_avg'`` / ``'.exp_avg_sq'``.  ``kind``: a dead fraction in [0, 1], ``"all_but_one"``, ``"all"`` or
    ``"hot"`` (one live row holding all the weight, every other row dead).  Rows violating the yardstick are resampled."""
    rng = np.random.default_rng(seed)
    if kind == "all":
        dead = np.ones(n, dtype=bool)
    elif kind in ("all_but_one", "hot"):
        dead = np.ones(n, dtype=bool)
        dead[(n * 2) // 3] = False
    else:
        dead = rng.uniform(size=n) < float(kind)
    logits = _logits(rng, n, dead)
    for _ in range(100):
        bad = violations(logits, min_opacity)
        if not bad.any():
            break
        logits = np.where(bad, _logits(rng, n, dead), logits)
    assert not violations(logits, min_opacity).any()
    W = {}
    for name in NAMES:
        W[name] = rng.standard_normal((n,) + SHAPES[name]).astype(np.float32)
        W[name + ".exp_avg"] = rng.standard_normal((n,) + SHAPES[name]).astype(np.float32)
        W[name + ".exp_avg_sq"] = rng.uniform(0.1, 1.0, (n,) + SHAPES[name]).astype(np.float32)
    W["opacity_logits"] = logits.reshape(n, 1)
    W["log_scales"] = rng.uniform(-5.0, -1.0, (n, 3)).astype(np.float32)
    return W


def expected_after(W: dict, n: int, phase: str, src, targets, values32) -> dict:
    """The 18 tensors after the contract's writes, from the oracle's draws and the engine-independent fp32 values."""
    src, targets = np.asarray(src, dtype=np.int64), np.asarray(targets, dtype=np.int64)
    k = src.shape[0]
    out = {}
    computed = {"opacity_logits": values32[:, :1], "log_scales": values32[:, 1:]}
    for name in NAMES:
        p = W[name]
        new = p.copy() if phase == "relocate" else np.concatenate([p, np.zeros((k,) + p.shape[1:], np.float32)])
        new[targets] = p[src]
        if name in computed:
            new[targets] = computed[name].reshape((k,) + p.shape[1:])
            new[src] = computed[name].reshape((k,) + p.shape[1:])
        out[name] = new
        for mom in (".exp_avg", ".exp_avg_sq"):
            m = W[name + mom]
            if phase == "relocate":
                m = m.copy()
                m[src] = 0.0
            else:
                m = np.concatenate([m, np.zeros((k,) + m.shape[1:], np.float32)])
            out[name + mom] = m
    return out
