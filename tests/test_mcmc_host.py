"""CPU: the MCMC refinement's torch engine (sgn_rast/mcmc.py) against the independent oracle (tests/mcmc_oracle.py),
stage by stage, and the strategy's schedule, cap, sampling statistics, deviates and optimiser handling.

Tolerances.  Integer stages (w, dead flags, src, targets, ratio) are EQUAL: the oracle's yardstick keeps every input an
fp64 rounding error away from a decision boundary.  New logits and log-scales: within 1 fp32 ulp of the oracle's fp64
value rounded to fp32, or 2^-30 absolute near 0 — one rounding plus the fp64 evaluation's own error, which
``test_fp64_formula_against_decimal`` holds below 1e-10 relative (measured: 2.3e-12 at logit 16, N = 51), three orders
under half an fp32 ulp."""
import math

import numpy as np
import pytest
import torch

import mcmc_oracle as O
from sgn_rast import mcmc

MIN_OP = 0.005


def _world(n, kind, seed=0, adam="stepped", cfg=None, engine_seed=3):
    W = O.make_world(n, kind, seed)
    P = {k: torch.from_numpy(W[k].copy()).requires_grad_(True) for k in O.NAMES}
    opt = {k: torch.optim.Adam([P[k]], lr=1.6e-4 if k == "means" else 1e-3) for k in P}
    if adam == "stepped":
        for k in P:
            opt[k].state[P[k]] = dict(step=torch.tensor(1.0), exp_avg=torch.from_numpy(W[k + ".exp_avg"].copy()),
                                      exp_avg_sq=torch.from_numpy(W[k + ".exp_avg_sq"].copy()))
    cfg = cfg or mcmc.MCMCConfig(warmup_length=0, refine_every=10, cap_max=10 ** 6)
    return W, P, opt, mcmc.MCMCDensifier(P, opt, cfg, seed=engine_seed)


def _tensors(D):
    out = {}
    for k in O.NAMES:
        out[k] = D.params[k].detach().numpy()
        st = D.optimizers[k].state.get(D.params[k], {})
        for mom in ("exp_avg", "exp_avg_sq"):
            if mom in st:
                out[k + "." + mom] = st[mom].numpy()
    return out


def _check_phase(W, n, stage, phase, key, n_max, k_grow=None):
    """One phase of an engine against the oracle; returns the expected 18 tensors after it."""
    assert not O.violations(W["opacity_logits"], MIN_OP).any()                    # the yardstick, first
    w, dead = O.weights(W["opacity_logits"], MIN_OP, relocate=phase == "relocate")
    assert np.array_equal(stage["w"].cpu().numpy().astype(np.int64), w)
    assert np.array_equal(stage["dead"].cpu().numpy().astype(bool), dead)
    k = int(dead.sum()) if phase == "relocate" else k_grow
    if k == 0 or w.sum() == 0:
        assert stage["src"].numel() == 0
        return {key_: v for key_, v in W.items()}
    src, ratio = O.draw(w, k, key, n_max)
    targets = np.nonzero(dead)[0] if phase == "relocate" else np.arange(n, n + k)
    assert np.array_equal(stage["src"].cpu().numpy().astype(np.int64), src)
    assert np.array_equal(stage["targets"].cpu().numpy().astype(np.int64), targets)
    assert np.array_equal(stage["ratio"].cpu().numpy().astype(np.int64), ratio)
    got = stage["values"].cpu().numpy()
    want = O.relocation_values64(W["opacity_logits"], W["log_scales"], src, ratio, MIN_OP)
    ok = O.within_ulp(got, want, 2.0 ** -30)
    assert ok.all(), (np.argwhere(~ok)[:5], got[~ok][:5], want[~ok][:5])
    return O.expected_after(W, n, phase, src, targets, got)


CASES = [(1, 0.0), (1, "all"), (257, 0.0), (257, 0.3), (257, "all"), (5000, 0.3), (5000, 0.0), (201, "hot")]


@pytest.mark.parametrize("n,kind", CASES)
def test_stage_by_stage_against_the_oracle(n, kind):
    W, P, opt, D = _world(n, kind, seed=n)
    before = {k: (P[k], opt[k].state[P[k]]["exp_avg"], opt[k].state[P[k]]["exp_avg_sq"]) for k in P}
    versions = {k: P[k]._version for k in P}
    relocated = D._phase(10, mcmc.RELOCATE)
    n_dead = int(O.weights(W["opacity_logits"], MIN_OP, True)[1].sum())
    skipped = n_dead == 0 or n_dead == n                     # no dead rows / all dead rows: the phase does nothing
    assert relocated == (0 if skipped else n_dead)
    exp = _check_phase(W, n, D.last["relocate"], "relocate", O.phase_key(3, 10, 1), 51)
    got = _tensors(D)
    for name, want in exp.items():                            # the writes AND every untouched row, over all 18 tensors
        assert np.array_equal(got[name].view(np.uint32), want.view(np.uint32)), name
    for k in P:                                               # in place: the same objects, versions bumped
        assert D.params[k] is before[k][0] and opt[k].state[P[k]]["exp_avg"] is before[k][1]
        assert opt[k].state[P[k]]["exp_avg_sq"] is before[k][2]
        if not skipped:
            assert P[k]._version > versions[k], k
    if kind == "hot":
        assert int(D.last["relocate"]["ratio"].max()) == 51 and n_dead == 200      # the ratio clamps at n_max
    # grow, on the weights after relocation
    k_grow = max(0, int(1.05 * n) - n)
    added = D._phase(10, mcmc.GROW)
    if k_grow == 0:
        assert added == 0 and "grow" not in D.last
        return
    exp2 = _check_phase(exp, n, D.last["grow"], "grow", O.phase_key(3, 10, 2), 51, k_grow=k_grow)
    total_w = int(O.weights(exp["opacity_logits"], MIN_OP, False)[0].sum())
    assert added == (k_grow if total_w else 0)
    got2 = _tensors(D)
    for name, want in exp2.items():
        assert got2[name].shape == want.shape, name
        assert np.array_equal(got2[name].view(np.uint32), want.view(np.uint32)), name
    if added:
        for k in P:                                           # new leaves, bound in their optimisers
            assert D.params[k] is not before[k][0] and D.params[k].requires_grad
            assert opt[k].param_groups[0]["params"][0] is D.params[k] and len(opt[k].state) == 1


def test_fp64_formula_against_decimal():
    worst = 0.0
    for logit in (-5.1, -2.0, 0.0, 3.0, 9.0, 16.0):
        for N in (2, 17, 51):
            _, ratio = O.relocation_decimal(logit, N)
            v = O.relocation_values64(np.array([logit], np.float32), np.zeros((1, 3), np.float32), np.array([0]),
                                      np.array([N]), MIN_OP)
            worst = max(worst, abs(math.exp(v[0, 1]) / float(ratio) - 1.0))
    print(f"fp64 o/S against 60-digit decimal: worst relative error {worst:.2e}")
    assert worst < 1e-10


def test_schedule_and_cap():
    cfg = mcmc.MCMCConfig(warmup_length=100, refine_every=100, stop_at=650, cap_max=1200)
    W, P, opt, D = _world(1000, 0.1, seed=5, cfg=cfg)
    counts, changed = [], []
    for step in range(200, 700, 100):
        changed.append(D.refinement_after(step))
        counts.append(D.params["means"].shape[0])
        assert D.record["gaussian_count"] == counts[-1] <= cfg.cap_max
    assert counts == [1050, 1102, 1157, 1200, 1200]
    assert changed == [True, True, True, True, False]
    assert D.record["added_count"] == 0
    # outside the window (warm-up, off-schedule, at / past stop_at) only the noise runs
    for step in (100, 50, 250, 650, 700):
        snap = {k: v.copy() for k, v in _tensors(D).items()}
        rec = dict(D.record)
        assert D.refinement_after(step) is False
        now = _tensors(D)
        assert not np.array_equal(now["means"], snap["means"])
        for name in snap:
            if name != "means":
                assert np.array_equal(now[name].view(np.uint32), snap[name].view(np.uint32)), (step, name)
        assert D.record == rec
    assert cfg.absgrad is False
    with pytest.raises(AttributeError):
        cfg.absgrad = True


def test_sampling_frequencies():
    """200 000 draws over 16 weights: every row's frequency within 5 binomial sigma (deterministic given the key)."""
    w = torch.tensor([1, 5, 0, 100, 7, 7, 2 ** 24, 3 * 2 ** 22, 12345, 1, 0, 999999, 31, 2 ** 23, 17, 4000000])
    k, total = 200_000, int(w.sum())
    src, _ = mcmc.draw(w, k, mcmc.phase_key(11, 300, mcmc.GROW), 51)
    freq = torch.bincount(src, minlength=16).double()
    p = w.double() / total
    sigma = torch.sqrt(k * p * (1 - p))
    dev = (freq - k * p).abs()
    assert bool((freq[w == 0] == 0).all())
    assert bool((dev <= 5 * sigma + 1e-9).all()), (dev / sigma.clamp(min=1e-9)).tolist()


def test_deviates_against_the_oracle_and_moments():
    n, key = 1_000_000, O.phase_key(4, 77, 3)
    z = mcmc.hash_normals(torch.arange(n), O.signed(key)).numpy()
    ok = O.within_ulp(z, O.normals64(np.arange(n), key), 2.0 ** -40)
    assert ok.all(), np.argwhere(~ok)[:5]
    m = z.size
    mean, var = float(z.astype(np.float64).mean()), float(z.astype(np.float64).var())
    assert abs(mean) < 5.0 / math.sqrt(m)                     # sigma of the mean of m unit normals
    assert abs(var - 1.0) < 5.0 * math.sqrt(2.0 / m)          # sigma of their sample variance
    # three distinct deviates a row, and another key gives other numbers
    assert not np.array_equal(z[:, 0], z[:, 2])
    assert not np.array_equal(z[:100], mcmc.hash_normals(torch.arange(100), O.signed(O.phase_key(4, 78, 3))).numpy())


def test_noise_follows_the_formula():
    W, P, opt, D = _world(300, 0.3, seed=9)
    with torch.no_grad():
        P["opacity_logits"].copy_(torch.linspace(-7, 7, 300)[:, None])
    old = P["means"].detach().clone()
    ver = P["means"]._version
    z = torch.empty(300, 3)
    D.inject_noise(40, z_out=z)
    assert P["means"]._version > ver
    scaler = 1.6e-4 * D.cfg.noise_lr
    d, norm, g = O.noise64(z.numpy(), P["log_scales"].detach().numpy(), P["quats"].detach().numpy(),
                           P["opacity_logits"].detach().numpy(), scaler)
    assert np.array_equal(z.numpy(), mcmc.hash_normals(torch.arange(300), mcmc.phase_key(3, 40, 3)).numpy())
    got = (P["means"].detach() - old).double().numpy()
    # fp32 formula + the rounding of the sum into means (|means| ~ 1): loose here, the GPU test holds the tight bound
    assert np.all(np.abs(got - d) <= 1e-4 * norm[:, None] + 2.0 ** -22 * (1 + np.abs(old.numpy())))
    assert g.min() < 1e-30 and g.max() > 0.6                  # the gate spans 0 to its top, sigmoid(0.5) = 0.62


@pytest.mark.parametrize("adam", ["fresh", "stepped"])
def test_optimisers_with_and_without_state(adam):
    W, P, opt, D = _world(257, 0.3, seed=2, adam=adam, cfg=mcmc.MCMCConfig(warmup_length=0, refine_every=10))
    assert D.refinement_after(10) is True
    n = D.params["means"].shape[0]
    assert n == int(1.05 * 257) and D.record == dict(relocated_count=D.record["relocated_count"], added_count=n - 257,
                                                      gaussian_count=n)
    for k in O.NAMES:                                         # Adam steps on the rebound parameters
        st = opt[k].state.get(D.params[k], {})
        assert ("exp_avg" in st) == (adam == "stepped")
        if adam == "stepped":
            assert st["exp_avg"].shape == D.params[k].shape and bool((st["exp_avg"][257:] == 0).all())
        D.params[k].grad = torch.ones_like(D.params[k])
        opt[k].step()
        assert opt[k].state[D.params[k]]["exp_avg"].shape == D.params[k].shape


def test_regularizer_and_protocol():
    W, P, opt, D = _world(50, 0.3, seed=1)
    c = D.cfg
    want = c.opacity_reg * torch.sigmoid(P["opacity_logits"]).mean() + c.scale_reg * torch.exp(P["log_scales"]).mean()
    r = D.regularizer()
    assert r.requires_grad and torch.equal(r, want)
    assert D.after_train(3, None, torch.zeros(50, dtype=torch.int32), (8, 8), absgrad=None) is None
    with pytest.raises(ValueError, match="engine"):
        mcmc.MCMCDensifier(P, opt, engine="triton")
    with pytest.raises(ValueError, match="n_max"):
        mcmc.MCMCDensifier(P, opt, mcmc.MCMCConfig(n_max=52))
    assert (c.warmup_length, c.refine_every) == (0, 10)
    d = mcmc.MCMCConfig()
    assert (d.warmup_length, d.refine_every, d.stop_at, d.cap_max, d.growth, d.min_opacity, d.noise_lr, d.n_max,
            d.opacity_reg, d.scale_reg) == (500, 100, 25000, 1_000_000, 1.05, 0.005, 5e5, 51, 0.01, 0.01)
