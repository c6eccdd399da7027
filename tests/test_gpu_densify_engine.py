"""GPU: `Densifier(engine="hip")` (csrc/densify.hip: decide / scan / apply) against the torch engine run on the CPU in
the same test — the reference's behaviour bit for bit (tests/test_densify_reference.py) — on the same inputs and the same
noise (`rng_device="cpu"`): the same N', `changed`, `record`, row map, ids and optimiser layout; every copied row of all
18 tensors bit-exact; moment rows of new rows exactly zero.  Before any comparison each world is shown (in fp64, on the
CPU) to keep every decision quantity at least a relative 1e-5 away from its threshold, far above the fp32 rounding of
exp / sigmoid / divide, so the masks must match exactly and no row is excused."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_densify_reference as M  # noqa: E402
from test_densify_reference import _close_to_frozen  # noqa: E402

from sgn_rast import densify  # noqa: E402
from sgn_rast.densify import PARAM_NAMES  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _cfg(**kw):
    return densify.DensifyConfig(**{**dict(num_train_data=M.NUM_TRAIN), **M.CFG, **kw})


# ------------------------------------------------------------------------------------------------------ the yardstick
def decision_margin(raw, stats, cfg, step, last_size=(64, 96)):
    """Smallest relative distance |q / t - 1| of any (finite) decision quantity to its threshold, in fp64."""
    gn, vc, m2d = (t.double() for t in stats)
    size = torch.exp(raw["log_scales"].double()).max(dim=-1).values
    alpha = torch.sigmoid(raw["opacity_logits"].double()).flatten()
    pairs = [(gn / vc * 0.5 * max(last_size), cfg.densify_grad_thresh), (size, cfg.densify_size_thresh),
             (size / 1.6, cfg.densify_size_thresh), (size, cfg.cull_scale_thresh), (size / 1.6, cfg.cull_scale_thresh),
             (alpha, cfg.cull_alpha_thresh)]
    if step < cfg.stop_screen_size_at:
        pairs += [(m2d, cfg.split_screen_size), (m2d, cfg.cull_screen_size)]
    worst = math.inf
    for q, t in pairs:
        q = q[torch.isfinite(q)]
        if q.numel():
            worst = min(worst, float((q / t - 1.0).abs().min()))
    return worst


def build(raw, state, stats, device, engine, cfg, seed=M.SEED, optim="adam", split_noise="stream"):
    """A Densifier over copies of the given inputs on `device` (state None: an optimiser that has not stepped yet)."""
    P = {k: torch.nn.Parameter(v.clone().to(device)) for k, v in raw.items()}
    if optim == "fused":
        from sgn_rast.optim import FusedAdam
        opts = {k: FusedAdam([P[k]], lr=1e-3, eps=1e-15) for k in P}
    else:
        opts = {k: torch.optim.Adam([P[k]], lr=1e-3, eps=1e-15) for k in P}
    if state is not None:
        for k in P:
            opts[k].state[P[k]] = {"step": torch.tensor(7.0), "exp_avg": state[k][0].clone().to(device),
                                   "exp_avg_sq": state[k][1].clone().to(device)}
    S = densify.Stats()
    if stats is not None:
        S.xys_grad_norm, S.vis_counts, S.max_2Dsize = (t.clone().to(device) for t in stats)
    D = densify.Densifier(P, opts, cfg, seed=seed, stats=S, rng_device="cpu", split_noise=split_noise, engine=engine)
    D.last_size = (64, 96)
    return D, opts


def tensors18(D, opts):
    """{name/param|exp_avg|exp_avg_sq: CPU tensor} (the moments only where the optimiser has them)."""
    out = {}
    for k in PARAM_NAMES:
        p = D.params[k]
        out[f"{k}/param"] = p.detach().cpu()
        st = opts[k].state.get(p, {})
        assert opts[k].param_groups[0]["params"][0] is p and len(opts[k].state) == 1
        for key in ("exp_avg", "exp_avg_sq"):
            if key in st:
                assert st[key].shape == p.shape
                out[f"{k}/{key}"] = st[key].cpu()
    return out


def implied_map(raw, ref):
    """(src, child, dup) of every output row of the torch engine: features_dc rows are bit-exact copies of their source
    row whatever the row is; new rows have zero moments (the inputs' second moments are positive), or, where the
    optimiser has no state, start at the first child (the children follow the kept originals); a duplicate repeats its
    parent's mean, a child does not."""
    def key(t):                                     # the bits of a row's first two floats (unique per input row)
        b = t.reshape(t.shape[0], -1)[:, :2].contiguous().view(torch.int32).long()
        return (b[:, 0] << 32) | (b[:, 1] & 0xFFFFFFFF)
    keys, order = key(raw["features_dc"]).sort()
    assert bool((keys[1:] != keys[:-1]).all())
    at = torch.searchsorted(keys, key(ref["features_dc/param"])).clamp(max=keys.numel() - 1)
    src = order[at].to(torch.int32)
    assert torch.equal(raw["features_dc"][src.long()], ref["features_dc/param"])
    same_mean = (ref["means/param"] == raw["means"][src.long()]).all(dim=-1)
    if "features_dc/exp_avg_sq" in ref:
        new = (ref["features_dc/exp_avg_sq"].flatten(1) == 0).all(dim=1)
    else:
        moved = (~same_mean).nonzero().flatten()
        start = int(moved[0]) if moved.numel() else src.numel()
        assert moved.numel() or bool((src[1:] > src[:-1]).all())              # no children: no duplicates either
        new = torch.arange(src.numel()) >= start
    return src, new & ~same_mean, new & same_mean


def compare(raw, state, stats, cfg, step, optim="adam", split_noise="stream", frozen=None, need=()):
    """Both engines on the same inputs; returns (hip Densifier, its optimisers, hip tensors, reference tensors)."""
    if stats is not None:
        margin = decision_margin(raw, stats, cfg, step)
        assert margin > 1e-5, margin
    Dr, or_ = build(raw, state, stats, "cpu", "torch", cfg, split_noise=split_noise)
    Dh, oh = build(raw, state, stats, DEV, "hip", cfg, optim=optim, split_noise=split_noise)
    changed_ref, changed = Dr.refinement_after(step), Dh.refinement_after(step)
    torch.cuda.synchronize()
    print(f"step {step}: N {raw['means'].shape[0]} -> {Dr.params['means'].shape[0]} (hip {Dh.params['means'].shape[0]})"
          f" record {Dr.record} (hip {Dh.record})")
    assert changed == changed_ref and Dh.record == Dr.record
    for key in need:
        assert Dr.record.get(key, 0) > 0, (key, Dr.record)
    ref, got = tensors18(Dr, or_), tensors18(Dh, oh)
    assert set(ref) == set(got)
    assert got["means/param"].shape[0] == ref["means/param"].shape[0]
    assert Dh.stats.xys_grad_norm is None
    for k in PARAM_NAMES:
        assert isinstance(Dh.params[k], torch.nn.Parameter) and Dh.params[k].is_cuda
    if not changed_ref:
        for key in ref:
            if key == "opacity_logits/param":
                # the opacity reset stays in torch on both sides: the clamp value is torch.logit evaluated on each
                # side's own device (one rounding of a value of magnitude 1.7); untouched rows are bit-exact
                same = ref[key] == raw["opacity_logits"]
                assert torch.equal(got[key][same], raw["opacity_logits"][same])
                assert float((ref[key] - got[key]).abs().max()) <= 2.0 ** -22 * float(ref[key].abs().max()), key
            else:
                assert torch.equal(ref[key], got[key]), key
        return Dh, oh, got, ref
    n_out = ref["means/param"].shape[0]
    if n_out == 0:
        assert Dh.last_src.numel() == 0 and Dh.ids.numel() == 0
        for key in ref:
            assert ref[key].shape == got[key].shape and ref[key].dtype == got[key].dtype, key
        return Dh, oh, got, ref
    src, child, dup = implied_map(raw, ref)
    kind = Dh.last_kind.cpu()
    assert torch.equal(Dh.last_src.cpu(), src)
    assert torch.equal(kind > 0, child) and torch.equal(kind < 0, dup)
    assert torch.equal(Dh.ids.cpu(), Dr.ids)
    # rows that are computed: child means; log_scales of children and of the duplicate of a split parent
    parents = torch.zeros(raw["means"].shape[0], dtype=torch.bool)
    parents[src[child].long()] = True
    shrunk = child | (dup & parents[src.long()])
    for key in ref:
        assert ref[key].shape == got[key].shape and ref[key].dtype == got[key].dtype, key
        name, what = key.split("/")
        exact = torch.ones(n_out, dtype=torch.bool)
        if what == "param" and name == "means":
            exact = ~child
        elif what == "param" and name == "log_scales":
            exact = ~shrunk
        assert torch.equal(ref[key][exact], got[key][exact]), key
        if what == "param":
            inp = raw[name][src.long()]
            assert torch.equal(got[key][exact], inp[exact]), key              # bit-exact copies of their source row
            if not bool(exact.all()):
                tol = 1e-6 * float(ref[key].abs().max())                      # the frozen file's bound (a few ulps)
                assert float((ref[key] - got[key]).abs().max()) <= tol, key
        else:
            assert float(got[key][child | dup].abs().sum()) == 0.0, key       # moments of new rows: exactly zero
            if state is not None:
                assert torch.equal(got[key][~(child | dup)], state[name][what == "exp_avg_sq"][src.long()][~(child | dup)])
    if frozen is not None:
        for key in got:
            _close_to_frozen(got[key], frozen[key], key)
    return Dh, oh, got, ref


def step_optimisers(D, opts):
    for k in D.params:
        D.params[k].grad = torch.ones_like(D.params[k])
    if all(type(o).__name__ == "FusedAdam" for o in opts.values()):
        from sgn_rast.optim import step_many
        step_many(opts.values())
    else:
        for o in opts.values():
            o.step()
    torch.cuda.synchronize()
    for k in D.params:
        assert bool(torch.isfinite(D.params[k]).all())


# ---------------------------------------------------------------------------------------------------- 1. golden world
@pytest.mark.parametrize("step", [15, 45, 40, 1005])
def test_golden_world(step):
    """n = 1500: split + dup + cull (15: 2197 rows), + screen-size and too-big culls (45: 2073 rows), the opacity reset
    alone (40), the cull-only refinement after stop_split_at (1005)."""
    raw, state, stats = M.world()
    need = {15: ("refine_splits_count", "refine_dups_count"), 1005: ("refine_culls_toobigs_count",),
            45: ("refine_splits_count", "refine_dups_count", "refine_culls_toobigs_count")}.get(step, ())
    frozen = M.load(step) if step in (15, 45) else None
    D, opts, got, ref = compare(raw, state, stats, _cfg(), step, optim="fused", frozen=frozen, need=need)
    if step == 15:
        assert got["means/param"].shape[0] == 2197 and (D.last_kind < 0).sum().item() > 0
    if step == 45:
        assert got["means/param"].shape[0] == 2073
    if step == 40:
        assert D.params["means"].shape[0] == 1500
        assert float(opts["opacity_logits"].state[D.params["opacity_logits"]]["exp_avg"].abs().max()) == 0.0
    if step == 1005:
        assert 0 < D.params["means"].shape[0] < 1500 and int(D.last_kind.abs().max()) == 0
    step_optimisers(D, opts)


@pytest.mark.parametrize("step", [15, 45])
def test_golden_world_hashed_ids_and_plain_adam(step):
    """`split_noise="hashed"`: persistent ids (children and duplicates derive theirs) equal the torch engine's; and
    torch.optim.Adam state."""
    raw, state, stats = M.world()
    D, opts, _, _ = compare(raw, state, stats, _cfg(), step, split_noise="hashed")
    assert D.ids.unique().numel() == D.ids.numel()
    step_optimisers(D, opts)


# --------------------------------------------------------------------------------------------------- 2. computed rows
def test_computed_rows_against_fp64():
    """Child means and shrunk log_scales of both engines ON THE DEVICE against an fp64 evaluation of the same expressions
    from the same fp32 inputs: the HIP engine's max-abs error is at most 4x the torch engine's (a dozen correctly rounded
    fp32 operations in possibly different association), with a floor of 2^-23 x the array's largest magnitude.
    Measured on the MI355X (golden world, step 15): means 2.67e-7 for both engines, log_scales 4.53e-7 for both —
    ratio 1.000 each (floors 6.06e-7 / 6.05e-7)."""
    raw, state, stats = M.world()
    cfg, step = _cfg(), 15
    assert decision_margin(raw, stats, cfg, step) > 1e-5
    Dt, ot = build(raw, state, stats, DEV, "torch", cfg)
    Dh, oh = build(raw, state, stats, DEV, "hip", cfg)
    assert Dt.refinement_after(step) and Dh.refinement_after(step)
    assert Dt.record == Dh.record and Dt.params["means"].shape == Dh.params["means"].shape
    src, kind = Dh.last_src.cpu().long(), Dh.last_kind.cpu().long()
    child = kind > 0
    n_splits, samps = Dh.record["refine_splits_count"], cfg.n_split_samples
    gen = torch.Generator().manual_seed((M.SEED * 1_000_003 + step) & 0x7FFFFFFFFFFFFFFF)
    noise = torch.randn((samps * n_splits, 3), generator=gen).double()
    # ---- fp64, the expressions of Densifier._split
    s = src[child]
    q = raw["quats"].double()[s]
    q = q / q.norm(dim=-1, keepdim=True)
    w, x, y, z = torch.unbind(torch.nn.functional.normalize(q, dim=-1), dim=-1)
    R = torch.stack([1 - 2 * (y**2 + z**2), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x**2 + z**2), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x**2 + y**2)], dim=-1).reshape(-1, 3, 3)
    scaled = torch.exp(raw["log_scales"].double()[s]) * noise[kind[child] - 1]
    means64 = torch.bmm(R, scaled[..., None]).squeeze(-1) + raw["means"].double()[s]
    parents = torch.zeros(raw["means"].shape[0], dtype=torch.bool)
    parents[s] = True
    shrunk = child | ((kind < 0) & parents[src])
    ls64 = torch.log(torch.exp(raw["log_scales"].double()[src[shrunk]]) / 1.6)
    assert int(child.sum()) > 500 and int(shrunk.sum()) > int(child.sum())
    for what, rows, want in (("means", child, means64), ("log_scales", shrunk, ls64)):
        err_hip = float((Dh.params[what].detach().cpu()[rows].double() - want).abs().max())
        err_torch = float((Dt.params[what].detach().cpu()[rows].double() - want).abs().max())
        floor = 2.0 ** -23 * float(want.abs().max())
        print(f"{what}: max|err| hip {err_hip:.3e} torch {err_torch:.3e} ratio {err_hip / max(err_torch, 1e-300):.3f} "
              f"floor {floor:.3e}")
        assert err_hip <= max(4.0 * err_torch, floor), (what, err_hip, err_torch, floor)


# ------------------------------------------------------------------------------------------------------------ 3. edges
def small_world(n, seed=3):
    raw, state, stats = M.world(n=n, seed=seed)
    return raw, state, stats


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_small_sizes(n):
    raw, state, stats = small_world(n)
    D, opts, _, _ = compare(raw, state, stats, _cfg(), 45)
    step_optimisers(D, opts)


def test_nothing_changes():
    """No row split, duplicated or culled: every tensor is a copy, `changed` is still what the torch engine says."""
    raw, state, stats = small_world(300)
    cfg = _cfg(densify_grad_thresh=1e9, cull_alpha_thresh=1e-9, cull_scale_thresh=1e9, cull_screen_size=1e9)
    D, _, got, _ = compare(raw, state, stats, cfg, 45)
    assert got["means/param"].shape[0] == 300 and torch.equal(got["means/param"], raw["means"])


@pytest.mark.parametrize("samps", [1, 2, 3])
def test_every_row_split(samps):
    raw, state, stats = small_world(300)
    cfg = _cfg(densify_grad_thresh=1e-12, densify_size_thresh=1e-9, cull_alpha_thresh=1e-9, n_split_samples=samps)
    D, opts, got, _ = compare(raw, None, stats, cfg, 15)                 # an optimiser that has no state yet
    assert D.record["refine_splits_count"] == 300 and got["means/param"].shape[0] == 300 * samps
    assert int((D.last_kind > 0).sum()) == 300 * samps and len(got) == 6
    step_optimisers(D, opts)


def test_every_row_culled():
    raw, state, stats = small_world(300)
    D, opts, got, _ = compare(raw, state, stats, _cfg(cull_alpha_thresh=1.0 - 1e-9), 45)
    assert all(t.shape[0] == 0 for t in got.values()) and len(got) == 18 and D.ids.numel() == 0


def test_unseen_rows():
    """vis_counts = 0: gradient 0 gives 0/0 = NaN (not high), gradient > 0 gives inf (high)."""
    raw, state, (gn, vc, m2d) = small_world(300)
    vc[:100] = 0.0
    gn[:50] = 0.0
    D, _, _, _ = compare(raw, state, (gn, vc, m2d), _cfg(), 15)
    # rows 50..99 are high whatever the threshold: each is split or duplicated
    high = torch.zeros(300, dtype=torch.bool)
    src, kind = D.last_src.cpu().long(), D.last_kind.cpu()
    high[src[kind != 0]] = True
    alive = torch.sigmoid(raw["opacity_logits"]).flatten() >= M.CFG["cull_alpha_thresh"]
    assert not bool(high[:50].any()) and bool(high[50:100][alive[50:100]].all())


def big_world(n=200_003, seed=9):
    """SH degree 3, every outcome frequent, and no decision quantity within 1 % of a threshold: rows that land closer
    are moved 1 % up (the thresholds of a quantity are far more than that apart)."""
    from sgn_rast import scenes
    cfg = _cfg()
    raw = scenes.make_gaussians(n, scenes.make_camera(96, 64, 80.0), seed=seed, z_range=(1.0, 5.0), sh_degree=3)
    g = torch.Generator().manual_seed(seed + 5)
    stats = [torch.rand(n, generator=g) * 0.0004, torch.randint(1, 6, (n,), generator=g).float(),
             torch.rand(n, generator=g) * 0.12]
    near = lambda q, ts: torch.stack([(q.double() / t - 1.0).abs() < 1e-3 for t in ts]).any(dim=0)
    size = torch.exp(raw["log_scales"].double()).max(dim=-1).values
    bump = near(size, (cfg.densify_size_thresh, cfg.cull_scale_thresh, 1.6 * cfg.densify_size_thresh,
                       1.6 * cfg.cull_scale_thresh))
    raw["log_scales"][bump] += math.log(1.01)
    stats[0][near(stats[0].double() / stats[1].double() * 0.5 * 96, (cfg.densify_grad_thresh,))] *= 1.01
    stats[2][near(stats[2], (cfg.split_screen_size, cfg.cull_screen_size))] *= 1.01
    alpha = torch.sigmoid(raw["opacity_logits"].double()).flatten()
    raw["opacity_logits"][near(alpha, (cfg.cull_alpha_thresh,))] += 0.05
    state = {k: (torch.randn(v.shape, generator=g) * 1e-3, torch.rand(v.shape, generator=g) * 1e-6)
             for k, v in raw.items()}
    return raw, state, tuple(stats), cfg


def test_many_blocks_sh3():
    """n = 200 003 at SH degree 3: several blocks of every kernel and of the scan, no multiple of any block size."""
    raw, state, stats, cfg = big_world()
    assert raw["features_rest"].shape[1:] == (15, 3)
    D, opts, got, _ = compare(raw, state, stats, cfg, 45, optim="fused",
                              need=("refine_splits_count", "refine_dups_count", "refine_culls_toobigs_count"))
    kind = D.last_kind
    assert int((kind == 0).sum()) > 10_000 and int((kind > 0).sum()) > 10_000 and int((kind < 0).sum()) > 10_000


# ----------------------------------------------------------------------------------------------------- 4. determinism
def test_two_runs_are_bit_identical():
    raw, state, stats = M.world()
    outs = []
    for _ in range(2):
        D, opts = build(raw, state, stats, DEV, "hip", _cfg())
        assert D.refinement_after(45)
        outs.append({**tensors18(D, opts), "src": D.last_src.cpu(), "kind": D.last_kind.cpu(), "ids": D.ids.cpu()})
    assert len(outs[0]) == 21
    for key in outs[0]:
        assert torch.equal(outs[0][key], outs[1][key]), key


# ------------------------------------------------------------------------------------------------------ 5. scene graph
def test_scene_graph():
    """Three sub-models over shared per-name optimisers; the middle one has no statistics and stays as it is."""
    worlds = [M.world(n=n, seed=s) for n, s in ((130, 1), (70, 2), (257, 3))]
    for (raw, _, stats), has in zip(worlds, (True, False, True)):
        assert not has or decision_margin(raw, stats, _cfg(), 15) > 1e-5

    def run(device, engine):
        models = [{k: torch.nn.Parameter(v.clone().to(device)) for k, v in raw.items()} for raw, _, _ in worlds]
        opts = {k: torch.optim.Adam([m[k] for m in models], lr=1e-3, eps=1e-15) for k in PARAM_NAMES}
        for m, (_, state, _) in zip(models, worlds):
            for k in PARAM_NAMES:
                opts[k].state[m[k]] = {"step": torch.tensor(7.0), "exp_avg": state[k][0].clone().to(device),
                                       "exp_avg_sq": state[k][1].clone().to(device)}
        G = densify.SceneGraphDensifier(models, opts, _cfg(), seed=M.SEED, rng_device="cpu", engine=engine)
        for i, (part, (_, _, stats)) in enumerate(zip(G.parts, worlds)):
            assert part.engine == engine
            part.last_size = (64, 96)
            if i != 1:
                part.stats.xys_grad_norm, part.stats.vis_counts, part.stats.max_2Dsize = (t.clone().to(device)
                                                                                          for t in stats)
        changed = G.refinement_after(15)
        layout = {}
        for k in PARAM_NAMES:
            group = opts[k].param_groups[0]["params"]
            assert len(group) == 3 and len(opts[k].state) == 3
            for i, p in enumerate(group):
                assert p is G.models[i][k] and p is G.parts[i].params[k]       # model order kept, addressed by identity
                layout[f"{k}/{i}"] = (p.detach().cpu(), opts[k].state[p]["exp_avg"].cpu(), opts[k].state[p]["exp_avg_sq"].cpu())
        return changed, layout, [p.record for p in G.parts], [p.ids.cpu() for p in G.parts], G, opts

    changed_ref, ref, rec_ref, ids_ref, _, _ = run("cpu", "torch")
    changed, got, rec, ids, G, opts = run(DEV, "hip")
    assert changed == changed_ref == [True, False, True] and rec == rec_ref
    assert all(torch.equal(a, b) for a, b in zip(ids, ids_ref))
    for key in ref:
        for a, b, what in zip(ref[key], got[key], ("param", "exp_avg", "exp_avg_sq")):
            assert a.shape == b.shape, (key, what)
            if what != "param" or key.split("/")[0] not in ("means", "log_scales"):
                assert torch.equal(a, b), (key, what)
            else:                                                              # computed rows: a few ulps (test 2)
                assert float((a - b).abs().max()) <= 1e-6 * float(a.abs().max()), (key, what)
    assert torch.equal(got["means/1"][0], worlds[1][0]["means"])
    for k in PARAM_NAMES:
        for p in opts[k].param_groups[0]["params"]:
            p.grad = torch.ones_like(p)
        opts[k].step()
