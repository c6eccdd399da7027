"""CPU: the rasterize node's depth-channel decision (`ops._depth_plan`) equals the expressions it was lifted from, for
every combination of its inputs, and the bookkeeping after a forward (`ops._settle_depth`) does per route what the node
did when each route carried its own copy of it — the differences between the routes included."""
import collections
import itertools
import types

import pytest

from sgn_rast import ops

H, W, N = 4, 6, 5


def _transcribed(win, id_range, num_points, cull, hit, want_depth, group_split, depth_channel, dcache, colors_shape,
                 colors_are_depths, depth_wanted):
    """`_RasterizeGaussians.forward` of the commit before `_depth_plan` existed (c334424), sgn_rast/ops.py lines
    1709-1725, name for name; `colors_c.shape` is `colors_shape`, `_depth_wanted()` is `depth_wanted()`."""
    img_height, img_width = H, W
    plain = win is None and id_range is None and num_points > 0 and cull                                       # :1709
    reuse = (plain and hit and not want_depth and group_split is None and depth_channel != "off" and dcache is not None
             and colors_shape == (num_points, 3) and dcache["D"].shape == (img_height, img_width))        # :1711-1712
    explicit = bool(want_depth) and win is None and num_points > 0                                             # :1720
    accumulate = (not reuse) and (explicit or (plain and not hit and depth_wanted()))                          # :1721
    depth_cacheable = accumulate and plain and not hit                                                         # :1722
    proved = bool(reuse and colors_are_depths)                                                                 # :1725
    return plain, reuse, proved, explicit, accumulate, depth_cacheable


def test_depth_plan_equals_the_expressions_it_replaces():
    seen = set()
    for (window, ranged, points, cull, hit, want, ungrouped, entry, rgb, are_depths,
         wanted) in itertools.product((False, True), repeat=11):
        for mode in ("auto", "on", "off"):
            plan = ops._depth_plan(window, ranged, points, cull, hit, want, ungrouped, mode, entry, rgb, are_depths,
                                   wanted)
            num_points = N if points else 0
            old = _transcribed(win=(0, None, 2 * N) if window else None, id_range=(0, 1) if ranged else None,
                               num_points=num_points, cull=cull, hit=hit, want_depth=want,
                               group_split=None if ungrouped else 2, depth_channel=mode,
                               dcache=dict(D=types.SimpleNamespace(shape=(H, W))) if entry else None,
                               colors_shape=(num_points, 3) if rgb else (num_points, 4),
                               colors_are_depths=are_depths, depth_wanted=lambda: wanted)
            assert tuple(plan) == tuple(bool(v) for v in old), (window, ranged, points, cull, hit, want, ungrouped,
                                                                entry, rgb, are_depths, wanted, mode)
            assert all(type(v) is bool for v in plan)
            seen.add(tuple(plan))
    with pytest.raises(AttributeError):
        plan.reuse = True                                   # immutable
    # the decision has exactly these outcomes (plain, reuse, proved, explicit, accumulate, cacheable)
    assert seen == {(False,) * 6, (True, False, False, False, False, False), (True, True, False, False, False, False),
                    (True, True, True, False, False, False), (True, False, False, False, True, True),
                    (True, False, False, True, True, True), (True, False, False, True, True, False),
                    (False, False, False, True, True, False)}


def _plan(**on):
    return ops._DepthPlan(**{**dict.fromkeys(ops._DepthPlan._fields, False), **on})


NONE = _plan()
IDLE = _plan(plain=True)                                            # a plain pass the policy does not accumulate on
FIRST = _plan(plain=True, accumulate=True, cacheable=True)          # "auto" / "on": a plain, freshly binned pass
ASKED = _plan(plain=True, explicit=True, accumulate=True, cacheable=True)       # want_depth on such a pass
ASKED_CACHED = _plan(plain=True, explicit=True, accumulate=True)    # want_depth on a cached list
ASKED_ODD = _plan(explicit=True, accumulate=True)                   # want_depth with an id_range / culling off
REUSE = _plan(plain=True, reuse=True)
PROVED = _plan(plain=True, reuse=True, proved=True)

# (route, plan, hit, num_intersects) -> (depth_stats deltas, cache action, "unused" reset to 0)
SETTLE = [
    # the one-call window route: nothing
    (ops._WINDOW, NONE, False, 7, {}, None, False),
    # the one-call fresh route: keep with the channel and something visible — else pop, nothing visible included
    (ops._FRESH, FIRST, False, 7, {"accumulated": 1}, ("remember", True), False),
    (ops._FRESH, ASKED, False, 7, {"accumulated": 1}, ("remember", True), False),
    (ops._FRESH, FIRST, False, 0, {}, "pop", False),
    (ops._FRESH, IDLE, False, 7, {}, "pop", False),
    (ops._FRESH, IDLE, False, 0, {}, "pop", False),
    # call by call, nothing visible: nothing at all, not even the pop
    (ops._NOTHING, FIRST, False, 0, {}, None, False),
    (ops._NOTHING, IDLE, False, 0, {}, None, False),
    (ops._NOTHING, IDLE, True, 0, {}, None, False),
    (ops._NOTHING, ASKED_ODD, False, 0, {}, None, False),
    (ops._NOTHING, PROVED, True, 0, {}, None, False),
    # call by call, groups: count; keep (not as a first pass) if cacheable, else pop on a fresh binning
    (ops._GROUPS, FIRST, False, 7, {"accumulated": 1}, ("remember", False), False),
    (ops._GROUPS, ASKED, False, 7, {"accumulated": 1}, ("remember", False), False),
    (ops._GROUPS, ASKED_CACHED, True, 7, {"accumulated": 1}, None, False),
    (ops._GROUPS, ASKED_ODD, False, 7, {"accumulated": 1}, "pop", False),
    (ops._GROUPS, ASKED_ODD, True, 7, {"accumulated": 1}, None, False),
    (ops._GROUPS, IDLE, False, 7, {}, "pop", False),
    (ops._GROUPS, IDLE, True, 7, {}, None, False),
    (ops._GROUPS, NONE, False, 7, {}, "pop", False),
    # call by call, plain
    (ops._PLAIN, REUSE, True, 7, {"reused": 1}, None, True),
    (ops._PLAIN, ASKED_CACHED, True, 7, {"accumulated": 1}, None, False),
    (ops._PLAIN, ASKED_ODD, True, 7, {"accumulated": 1}, None, False),
    (ops._PLAIN, ASKED_ODD, False, 7, {"accumulated": 1}, None, False),          # no pop although freshly binned
    (ops._PLAIN, FIRST, False, 7, {"accumulated": 1}, ("remember", True), False),
    (ops._PLAIN, ASKED, False, 7, {"accumulated": 1}, ("remember", True), False),
    (ops._PLAIN, IDLE, False, 7, {}, "pop", False),
    (ops._PLAIN, IDLE, True, 7, {}, None, False),
    (ops._PLAIN, NONE, False, 7, {}, "pop", False),                              # a matched window, culling off, ...
    (ops._PLAIN, NONE, True, 7, {}, None, False),
    # call by call, proven reuse
    (ops._PROVEN, PROVED, True, 7, {"reused": 1, "proved_on_host": 1}, None, True),
]


@pytest.mark.parametrize("route,plan,hit,num_intersects,deltas,action,resets", SETTLE)
def test_settle_depth_per_route(monkeypatch, route, plan, hit, num_intersects, deltas, action, resets):
    key = ("the", "key")
    S = types.SimpleNamespace(depth_caches=collections.OrderedDict([(key, "stale"), ("other", "entry")]),
                              depth_state={"want": True, "unused": 3, "cache": None})
    call = types.SimpleNamespace(out_depth="D", outs=("img", "T", "idx"))
    remembered = []
    monkeypatch.setattr(ops, "_remember_depth",
                        lambda S_, key_, D, T, idx, kmax, first_pass=True: remembered.append(
                            (S_ is S, key_, D, T, idx, kmax, first_pass)))
    before = dict(ops.depth_stats)
    monkeypatch.setattr(ops, "depth_stats", dict(before))
    ops._settle_depth(S, plan, route, key, hit, num_intersects, call, "kmax")
    assert {k: v - before[k] for k, v in ops.depth_stats.items() if v != before[k]} == deltas
    if isinstance(action, tuple):
        assert remembered == [(True, key, "D", "T", "idx", "kmax", action[1])]
        assert list(S.depth_caches) == [key, "other"]
    else:
        assert remembered == []
        assert list(S.depth_caches) == (["other"] if action == "pop" else [key, "other"])
    assert S.depth_state == {"want": True, "unused": 0 if resets else 3, "cache": None}


def test_remember_depth_counts_first_passes_only(monkeypatch):
    """What `first_pass` means to the "auto" policy: nine unused first-pass images switch the accumulation off again;
    a group pass's image (first_pass=False) is kept without counting."""
    S = types.SimpleNamespace(depth_caches=collections.OrderedDict(), depth_state={"want": True, "unused": 0})
    monkeypatch.setattr(ops, "depth_channel", "auto")
    for i in range(8):
        ops._remember_depth(S, "k", "D", "T", "idx", "kmax", first_pass=False)
        ops._remember_depth(S, "k", "D", "T", "idx", "kmax")
        assert S.depth_state == {"want": True, "unused": i + 1}
    ops._remember_depth(S, "k", "D", "T", "idx", "kmax")
    assert S.depth_state == {"want": False, "unused": 0} and list(S.depth_caches) == ["k"]
