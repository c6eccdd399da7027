"""Which library entry points the rasterize node calls, in which order, and which counters it moves — per scenario, over
a fixed list of small scenarios that between them take every route of `_RasterizeGaussians.forward` (one-call window,
one-call fresh, call by call: proven depth reuse, nothing visible, groups, plain with and without flagged reuse) and its
backward.  The output is text that depends on the host logic only: run it on two commits and compare the two outputs
byte for byte (profiles/raster_host.md).

The loaded library handle of `sgn_rast._lib` is replaced by a proxy that notes the NAME of every `sgn_*` entry point
called and forwards the call.  Scenes: 300 screen-space splats on a 40 x 64 image (the shape of
tests/test_gpu_onecall_transports.py), as a concatenation of two sub-models (240 + 60 rows) for the window passes."""
import hashlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, os.environ.get("PKG", "street-gaussians-ns_amd"))]
import torch
from sgn_rast import _lib as L, config, fused, ops

DEV = torch.device("cuda", 0)
H, W, BLOCK, N, N_HEAD = 40, 64, 16, 300, 240


def scene(kind="street", seed=11):
    """Screen-space splats (fixed seed, made on the CPU).  "street": small splats, one to four tiles each; "wide": every
    splat covers the image (more than 1.3 x the intersections of "street": a capacity miss); "blind": nothing visible."""
    g = torch.Generator().manual_seed(seed)
    xys = torch.rand(N, 2, generator=g) * torch.tensor([float(W), float(H)])
    sigma = 0.8 + 3.0 * torch.rand(N, generator=g)
    opac = 0.2 + 0.7 * torch.rand(N, generator=g)
    if kind == "wide":
        sigma = sigma * 0 + 40.0
    radii = torch.ceil(3.0 * sigma).to(torch.int32)
    if kind == "blind":
        radii = radii * 0
    conics = torch.stack([1.0 / sigma ** 2, 0.1 * (torch.rand(N, generator=g) - 0.5) / sigma ** 2, 1.0 / sigma ** 2], 1)
    r = radii.float()[:, None]
    grid = torch.tensor([W // BLOCK, (H + BLOCK - 1) // BLOCK], dtype=torch.int32)
    lo = torch.minimum(((xys - r) / BLOCK).to(torch.int32).clamp(min=0), grid)
    hi = torch.minimum(((xys + r) / BLOCK + 1.0).to(torch.int32).clamp(min=0), grid)
    nth = ((hi - lo).clamp(min=0).prod(1) * (radii > 0)).to(torch.int32)
    sc = dict(xys=xys, depths=1.0 + 9.0 * torch.rand(N, generator=g), radii=radii, conics=conics, nth=nth,
              colors=torch.rand(N, 3, generator=g), opac=opac, bg=torch.tensor([0.1, 0.2, 0.3]))
    return {k: v.contiguous().to(DEV) for k, v in sc.items()}


class Proxy:
    """The library handle with every `sgn_*` call noted by name."""
    def __init__(self, lib, names):
        self._lib, self._names, self._wrapped = lib, names, {}

    def __getattr__(self, k):
        f = self._wrapped.get(k)
        if f is None:
            inner, names = getattr(self._lib, k), self._names
            if not k.startswith("sgn_"):
                return inner

            def f(*a):
                names.append(k)
                return inner(*a)
            self._wrapped[k] = f
        return f


names = []
L.load()
L._lib = Proxy(L._lib, names)
STATS = {k: getattr(ops, k) for k in sorted(vars(ops)) if k.endswith("_stats") and isinstance(getattr(ops, k), dict)}
lines = []


def say(text):
    lines.append(text)
    print(text, flush=True)


def scenario(title, fn):
    names.clear()
    before = {k: dict(d) for k, d in STATS.items()}
    fn()
    torch.cuda.synchronize()
    say(f"## {title}")
    say("calls: " + " ".join(names))
    moved = [f"{k}.{key}: {before[k].get(key)} -> {v}" for k, d in STATS.items() for key, v in sorted(d.items())
             if before[k].get(key) != v]
    say("stats: " + ("; ".join(moved) or "-"))


def leaves(sc, rows=slice(None)):
    """Fresh tensors of rows `rows` of a scene (a new binning key), depths with a graph behind them (the proofs read it)."""
    t = {k: sc[k][rows].clone() for k in ("xys", "depths", "radii", "conics", "nth", "colors", "opac")}
    for k in ("xys", "conics", "colors", "opac"):
        t[k].requires_grad_(True)
    t["depths"] = t["depths"].requires_grad_(True) * 1.0
    t["bg"] = sc["bg"]
    return t


def dropin(t, colors=None):
    img, alpha = ops.rasterize_gaussians(t["xys"], t["depths"], t["radii"], t["conics"], t["nth"],
                                         t["colors"] if colors is None else colors, t["opac"], H, W, BLOCK, t["bg"], True)
    (img.sum() + 0.5 * alpha.sum()).backward(retain_graph=True)      # (the depth pass comes back to `depths`' graph)


def fused_call(t, **kw):
    out = fused.rasterize_gaussians_fused(t["xys"], t["depths"], t["radii"], t["conics"], t["nth"], t["colors"], t["opac"],
                                          H, W, BLOCK, t["bg"], True, **kw)
    sum(o.sum() for o in out if o is not None and o.requires_grad).backward(retain_graph=True)


def depth_pair(sc, title, provable):
    """A colour pass over fresh tensors, then the reference's depth pass over the same tensors."""
    t = leaves(sc)
    scenario(f"{title}: colour pass", lambda: dropin(t))
    d = t["depths"]
    colors = d[:, None].repeat(1, 3) if provable else torch.stack([d, d, d], 1)
    scenario(f"{title}: depth pass, colours {'provably' if provable else 'not provably'} the depths",
             lambda: dropin(t, colors))


def walk(tag):
    street, wide, blind = scene("street"), scene("wide"), scene("blind")
    say(f"# {tag}")
    ops.clear_binning_cache()
    ops._depth_state.update(want=False, unused=0)
    scenario("first call of this shape", lambda: dropin(leaves(street)))
    scenario("second call", lambda: dropin(leaves(street)))
    for provable in (True, False, True, False):                 # ("auto" starts accumulating after the first pair)
        depth_pair(street, "same tensors again", provable)
    for mode in ("on", "auto", "off"):
        with config.override(depth_channel=mode):
            ops._depth_state.update(want=False, unused=0)
            for provable in (True, False):
                depth_pair(street, f"depth_channel={mode}", provable)
    ops._depth_state.update(want=False, unused=0)
    t = leaves(street)
    scenario("fused, depth asked for, fresh list", lambda: fused_call(t, depth_channel=True))
    scenario("fused, depth asked for, cached list", lambda: fused_call(t, depth_channel=True))
    scenario("fused, depth asked for, id_range", lambda: fused_call(t, depth_channel=True, id_range=(0, 100)))
    scenario("group_split with depth, cached list", lambda: fused_call(t, depth_channel=True, group_split=N - 60))
    scenario("fused, id_range on a fresh list", lambda: fused_call(leaves(street), id_range=(100, 300)))
    scenario("window passes: the whole scene", lambda: dropin(leaves(street)))
    scenario("window passes: head sub-model (shared list)", lambda: dropin(leaves(street, slice(0, N_HEAD))))
    scenario("window passes: tail sub-model (sub-list)", lambda: dropin(leaves(street, slice(N_HEAD, N))))
    scenario("group_split, the small group on its own list", lambda: fused_call(leaves(street), group_split=N - 60))
    scenario("group_split, both groups on the shared list", lambda: fused_call(leaves(street), group_split=N // 2))
    scenario("group_split with depth, fresh list",
             lambda: fused_call(leaves(street), depth_channel=True, group_split=N - 60))
    scenario("a view that sees nothing", lambda: dropin(leaves(blind)))
    scenario("a view that sees nothing, depth asked for", lambda: fused_call(leaves(blind), depth_channel=True))
    scenario("capacity miss (more than 1.3 x the intersections seen)", lambda: dropin(leaves(wide)))
    scenario("the call after the miss", lambda: dropin(leaves(wide)))
    with config.override(tile_culling=False):
        scenario("tile_culling off", lambda: dropin(leaves(street)))
        scenario("tile_culling off, depth asked for", lambda: fused_call(leaves(street), depth_channel=True))
        scenario("tile_culling off, group_split with depth",
                 lambda: fused_call(leaves(street), depth_channel=True, group_split=N - 60))


walk("one_call_nodes=True")
with config.override(one_call_nodes=False):
    walk("one_call_nodes=False")
print("sha256 of the lines above:", hashlib.sha256("\n".join(lines).encode()).hexdigest())
