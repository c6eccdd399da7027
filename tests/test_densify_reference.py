"""CPU: `sgn_rast.densify.Densifier` against the REFERENCE's own `refinement_after` / `split_gaussians` /
`dup_gaussians` / `cull_gaussians` / `dup_in_optim` / `remove_from_optim` (sgn_splatfacto.py:459-720) on the same
parameters, optimiser state, statistics and random stream: new parameters and Adam moments must be BIT-IDENTICAL, for a
densifying step (split + dup + cull), one past the first opacity-reset interval (screen-size / too-big culls) and an
opacity-reset step.  Where the reference checkout exists it is executed literally (tests/refhost.py) and the port must
equal it bit for bit.  Everywhere, the port is also checked against the reference's outcome frozen in
tests/golden/densify_reference.npz (tests/golden/make_densify_reference.py): the same point count and shapes, and values
equal up to a few units in the last place (another host's vectorised CPU math may round differently from the one that
froze the file).  `tests/test_dp_gloo.py` covers the replicated (2-rank) behaviour."""
import os
import sys

import pytest
import torch

import refhost
from helpers import TorchStats

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_densify_reference as M  # noqa: E402

REF2OURS, CFG, SEED, NUM_TRAIN = M.REF2OURS, M.CFG, M.SEED, M.NUM_TRAIN
_world = M.world


def _close_to_frozen(got, want, what):
    """Same shape, values within 1e-6 of the array's largest magnitude (a few ulps), with the worst element on failure."""
    got, want = got.detach(), torch.from_numpy(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, tuple(got.shape), tuple(want.shape))
    tol = 1e-6 * float(want.abs().max())
    err = (got - want).abs()
    assert err.numel() == 0 or float(err.max()) <= tol, (what, float(err.max()), tol, int(err.argmax()))


@pytest.mark.parametrize("step", [15, 45, 40, 100])
def test_refinement_equals_the_reference_bit_for_bit(step):
    from sgn_rast import densify
    frozen = M.load(step)
    live = M.reference_outcome(step) if refhost.available() else None      # the reference, literally
    raw, state, stats = _world()
    # ---- the port
    P = {k: torch.nn.Parameter(v.clone()) for k, v in raw.items()}
    opts = {k: torch.optim.Adam([P[k]], lr=1e-3, eps=1e-15) for k in P}
    for k in P:
        opts[k].state[P[k]] = {"step": torch.tensor(7.0), "exp_avg": state[k][0].clone(),
                               "exp_avg_sq": state[k][1].clone()}
    S = TorchStats()
    S.xys_grad_norm, S.vis_counts, S.max_2Dsize = (t.clone() for t in stats)
    D = densify.Densifier(P, opts, densify.DensifyConfig(num_train_data=NUM_TRAIN, **CFG), seed=SEED, stats=S)
    D.last_size = (64, 96)
    changed = D.refinement_after(step)
    # ---- identical outcome
    n_ref = int(frozen["num_points"])
    assert live is None or int(live["num_points"]) == n_ref
    assert (n_ref != raw["means"].shape[0]) == changed
    assert D.params["means"].shape[0] == n_ref
    if step in (15, 45):
        assert changed and D.record["refine_splits_count"] > 0 and D.record["refine_dups_count"] > 0
    for ours in REF2OURS.values():
        p = D.params[ours]
        st = opts[ours].state[p]
        assert isinstance(p, torch.nn.Parameter)
        assert opts[ours].param_groups[0]["params"][0] is p and len(opts[ours].state) == 1
        for key, got in (("param", p.detach()), ("exp_avg", st["exp_avg"]), ("exp_avg_sq", st["exp_avg_sq"])):
            if live is not None:
                assert torch.equal(torch.from_numpy(live[f"{ours}/{key}"]), got), (ours, key)
            _close_to_frozen(got, frozen[f"{ours}/{key}"], (ours, key))
        assert st["exp_avg"].shape == p.shape
    assert S.xys_grad_norm is None
    if step == 40:       # opacity reset: clamped logits, zeroed moments
        assert float(torch.sigmoid(D.params["opacity_logits"]).max()) <= 0.16 + 1e-6
        assert float(opts["opacity_logits"].state[D.params["opacity_logits"]]["exp_avg"].abs().max()) == 0.0
    # an optimiser step on the new layout works (state and parameter agree in shape)
    for k in D.params:
        D.params[k].grad = torch.ones_like(D.params[k])
        opts[k].step()
