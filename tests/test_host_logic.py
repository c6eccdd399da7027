"""CPU: host-side logic of the operator surface (argument validation mirrors upstream gsplat's
error behaviour; helper functions; synthetic scenes; DP view sharding)."""
import pytest
import torch

from sgn_rast import dp, ops, scenes


def test_num_sh_bases_and_inverse():
    assert [ops.num_sh_bases(d) for d in range(5)] == [1, 4, 9, 16, 25]
    assert [ops.deg_from_sh(k) for k in (1, 4, 9, 16, 25)] == [0, 1, 2, 3, 4]
    with pytest.raises(AssertionError):
        ops.deg_from_sh(7)


def test_quat_to_rotmat_matches_oracle_and_is_orthonormal(torch_oracle):
    q = torch.randn(100, 4)
    R = ops.quat_to_rotmat(q)
    assert torch.allclose(R, torch_oracle.quat_to_rotmat(q))
    assert torch.allclose(R @ R.transpose(-1, -2), torch.eye(3).expand(100, 3, 3), atol=1e-5)
    assert torch.allclose(torch.linalg.det(R), torch.ones(100), atol=1e-5)
    assert torch.allclose(ops.quat_to_rotmat(torch.tensor([[2.0, 0, 0, 0]])), torch.eye(3)[None])


def test_rasterize_argument_validation_matches_upstream():
    n = 4
    good = dict(xys=torch.rand(n, 2), depths=torch.rand(n), radii=torch.ones(n, dtype=torch.int32),
                conics=torch.rand(n, 3), num_tiles_hit=torch.ones(n, dtype=torch.int32),
                colors=torch.rand(n, 3), opacity=torch.rand(n, 1))
    with pytest.raises(AssertionError, match="block_width must be between 2 and 16"):
        ops.rasterize_gaussians(*good.values(), 8, 8, 17)
    with pytest.raises(AssertionError, match="block_width must be between 2 and 16"):
        ops.rasterize_gaussians(*good.values(), 8, 8, 1)
    with pytest.raises(AssertionError, match="incorrect shape of background"):
        ops.rasterize_gaussians(*good.values(), 8, 8, 16, background=torch.zeros(4))
    bad = dict(good, xys=torch.rand(n, 3))
    with pytest.raises(ValueError, match=r"xys must have dimensions \(N, 2\)"):
        ops.rasterize_gaussians(*bad.values(), 8, 8, 16)
    bad = dict(good, colors=torch.rand(n, 3, 1))
    with pytest.raises(ValueError, match=r"colors must have dimensions \(N, D\)"):
        ops.rasterize_gaussians(*bad.values(), 8, 8, 16, background=torch.zeros(1))


def test_project_argument_validation_matches_upstream():
    n = 4
    q = torch.zeros(n, 4); q[:, 0] = 1
    args = [torch.rand(n, 3), torch.rand(n, 3), 1, q, torch.eye(4)[:3], 10., 10., 4., 4., 8, 8]
    with pytest.raises(AssertionError, match="block_width must be between 2 and 16"):
        ops.project_gaussians(*args, 32)
    args[3] = q * 2
    with pytest.raises(AssertionError, match="quats must be normalized"):
        ops.project_gaussians(*args, 16)
    args[3] = q
    args[0] = torch.rand(n, 2)
    with pytest.raises(ValueError, match="Invalid shape for means3d"):
        ops.project_gaussians(*args, 16)


def test_sh_argument_validation():
    with pytest.raises(AssertionError):
        ops.spherical_harmonics(3, torch.rand(4, 3), torch.rand(4, 9, 3))  # degree needs 16 bases
    with pytest.raises(AssertionError, match="Invalid method"):
        ops.spherical_harmonics(0, torch.rand(4, 3), torch.rand(4, 1, 3), method="nope")


def test_scenes_are_deterministic_and_match_spec():
    cam, P = scenes.make_scene("c1")
    cam2, P2 = scenes.make_scene("c1")
    assert all(torch.equal(P[k], P2[k]) for k in P)
    assert P["means"].shape == (10_000, 3) and P["features_rest"].shape == (10_000, 15, 3)
    assert cam.width == 128 and cam.fx == 128.0
    o = torch.sigmoid(P["opacity_logits"])
    assert 0.0199 < float(o.min()) and float(o.max()) < 0.9801
    s = P["log_scales"].exp()
    assert 0.0099 < float(s.min()) and float(s.max()) < 0.1001
    z = P["means"][:, 2]
    assert 1.0 <= float(z.min()) and float(z.max()) <= 5.0
    assert scenes.SCENES["metric"][:3] == (1_000_000, 1920, 1280)
    yawed = scenes.make_camera(64, 64, 64.0, yaw=0.3)
    R = yawed.viewmat[:3, :3]
    assert torch.allclose(R @ R.T, torch.eye(3), atol=1e-6)


def test_view_sharding_covers_every_view_once_per_epoch():
    n_views, world = 24, 8
    seen = []
    for step in range(n_views // world):
        seen += [dp.view_for_rank(step, r, world, n_views, seed=3) for r in range(world)]
    assert sorted(seen) == list(range(n_views))
    nxt = [dp.view_for_rank(n_views // world, r, world, n_views, seed=3) for r in range(world)]
    assert nxt != seen[:world]  # new permutation in the next epoch
    assert dp.view_for_rank(5, 2, 4, 10, seed=1) == dp.view_for_rank(5, 2, 4, 10, seed=1)


def test_dependency_shims_resolve_to_the_hip_modules():
    """The reference's imports (sgn_splatfacto.py:8, :11-15) resolve inside street-gaussians-ns_amd/."""
    import importlib
    dr = importlib.import_module("nvdiffrast.torch")
    ms = importlib.import_module("pytorch_msssim")
    from sgn_rast import loss, sky
    assert dr.texture is sky.texture and ms.SSIM is loss.SSIM
    mod = ms.SSIM(data_range=1.0, size_average=True, channel=3)          # the reference's constructor call (:330)
    assert mod.data_range == 1.0


def test_next_row_modules_validate_arguments_without_a_gpu():
    """sky / loss / optim / densify: argument errors are raised on the host, and CPU tensors are refused (no
    fallback) before anything touches the device."""
    from sgn_rast import _lib, densify, loss, optim, sky
    tex, uv = torch.rand(1, 6, 4, 4, 3), torch.rand(1, 2, 2, 3)
    with pytest.raises(NotImplementedError):
        sky.texture(tex, uv, filter_mode="nearest")
    with pytest.raises(NotImplementedError):
        sky.texture(tex, uv, boundary_mode="wrap")
    with pytest.raises(ValueError):
        sky.texture(torch.rand(1, 5, 4, 4, 3), uv)                  # not a cube map
    with pytest.raises(ValueError):
        sky.texture(tex, torch.rand(2, 2, 2, 3))                    # batch mismatch
    with pytest.raises(_lib.SgnRastError):
        sky.texture(tex, uv)                                        # CPU tensors: refused
    with pytest.raises(NotImplementedError):
        loss.SSIM(data_range=1.0, size_average=False)
    with pytest.raises(NotImplementedError):
        loss.SSIM(data_range=1.0, channel=1)
    with pytest.raises(ValueError):
        loss.SSIM(data_range=1.0)(torch.rand(2, 3, 16, 16), torch.rand(2, 3, 16, 16))   # batch 1 only
    with pytest.raises(_lib.SgnRastError):
        loss.l1_ssim(torch.rand(16, 16, 3), torch.rand(16, 16, 3))
    with pytest.raises(NotImplementedError):
        optim.FusedAdam([torch.zeros(3, requires_grad=True)], amsgrad=True)
    with pytest.raises(ValueError):
        optim.FusedAdam([torch.zeros(3, requires_grad=True)], lr=-1.0)
    p = torch.zeros(3, requires_grad=True)
    p.grad = torch.ones(3)
    with pytest.raises(_lib.SgnRastError):
        optim.FusedAdam([p]).step()
    with pytest.raises(_lib.SgnRastError):
        densify.Stats().update(torch.zeros(4, 2), torch.ones(4, dtype=torch.int32), (8, 8))
    # the state layout is torch.optim.Adam's (the reference's densification edits these tensors in place)
    o = optim.FusedAdam([torch.zeros(3, requires_grad=True)], lr=1e-3, eps=1e-15)
    assert o.param_groups[0]["eps"] == 1e-15 and o.param_groups[0]["betas"] == (0.9, 0.999)


def test_bench_cpu_baseline_leg_runs_without_a_gpu():
    """bench.py's bounded CPU-baseline sample (the oracle timed on the host cores) is a separate process that needs no
    GPU; its JSON carries the fields the bench line embeds."""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--cpu-baseline-only", "--scene", "c1",
                          "--cpu-rows", "1", "--cpu-frac", "4"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-500:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")][-1]
    d = json.loads(line)
    assert d["unit"] == "images/sec" and d["kind"] == "port" and d["value"] > 0 and d["cores"] >= 1
    assert "2500 of 10000 Gaussians" in d["sample"]
    # the two fully measured figures of the plain-C port: one core, and its compositing on all cores
    assert d["c_port"]["cores"] == 1 and d["c_port"]["value"] > 0 and "nothing extrapolated" in d["c_port"]["sample"]
    assert d["c_port_all_cores"]["cores"] >= 1 and d["c_port_all_cores"]["value"] > 0


def test_bench_dump_outputs_is_bounded_and_reproducible(tmp_path, monkeypatch):
    """bench.py --dump-outputs on outputs of the metric size (1 M Gaussians, 1920x1280) and of the scene graph (nine
    models, five images, the sky cube map's gradient): float32 / float64 files, at most 64 MB in all, the same seeded
    samples every time."""
    import os
    import sys
    from types import SimpleNamespace
    import numpy as np
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    # (importing bench.py sets this variable for its own process: put back as it was after the test)
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench
    H, W, N = 1280, 1920, 1_000_000
    cam = SimpleNamespace(height=H, width=W)
    g = torch.Generator().manual_seed(3)

    def leaf(*shape):
        p = torch.zeros(*shape, requires_grad=True)
        p.grad = torch.rand(*shape, generator=g)
        return p

    P = {k: leaf(N, *s) for k, s in dict(means=(3,), log_scales=(3,), quats=(4,), opacity_logits=(1,),
                                         features_dc=(1, 3), features_rest=(15, 3)).items()}
    out = SimpleNamespace(rgb=torch.rand(H, W, 3, generator=g), alpha=torch.rand(H, W, generator=g),
                          xys=torch.rand(N, 2, generator=g), radii=torch.randint(0, 9, (N,), dtype=torch.int32),
                          loss=torch.tensor(0.25))
    models = [{"means": leaf(N // 9, 3), "features_rest": leaf(N // 9, 15, 3)} for _ in range(9)]
    sg_out = SimpleNamespace(rgb=out.rgb, alpha=out.alpha, depth=torch.rand(H, W, 1, generator=g),
                             object_acc=out.alpha, background_acc=out.alpha, loss=out.loss,
                             radii=torch.zeros(9 * (N // 9), dtype=torch.int32))
    sky = {"base": leaf(6, 1024, 1024, 3)}
    for name, args in (("plain", (out, [P], cam)), ("scene_graph", (sg_out, models, cam, sky))):
        shapes = [bench.dump_outputs(str(tmp_path / f"{name}{i}"), *args) for i in range(2)]
        assert shapes[0] == shapes[1]
        files = sorted(os.listdir(tmp_path / f"{name}0"))
        assert files == sorted(n + ".npy" for n in shapes[0])
        assert sum(os.path.getsize(tmp_path / f"{name}0" / f) for f in files) <= 64 * 10**6
        for f in files:
            a, b = np.load(tmp_path / f"{name}0" / f), np.load(tmp_path / f"{name}1" / f)
            assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f
    plain = bench.dump_outputs(str(tmp_path / "plain0"), out, [P], cam)
    assert plain["rgb"] == [H, W, 3] and plain["alpha"] == [H, W]            # the images whole, the rest sampled
    assert plain["grad_features_rest"] == [bench.DUMP_ROWS, 15, 3] and plain["loss"] == []
    rows = np.load(tmp_path / "plain0" / "rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "plain0" / "grad_means.npy"), P["means"].grad[rows].numpy())


def test_quaternion_multiply_shim_on_cpu_is_pytorch3d_formula():
    """`from pytorch3d.transforms import quaternion_multiply` resolves to the product shim; with CPU operands (the
    reference's bbox optimiser, data/utils/bbox_optimizers.py:155-161) it is pytorch3d's plain-torch formulation: Hamilton
    product, real part first, standardised sign, float64 0-dim scalars do not promote a float32 tensor."""
    import importlib
    import sys
    saved = sys.modules.pop("pytorch3d", None), sys.modules.pop("pytorch3d.transforms", None)
    try:
        T = importlib.import_module("pytorch3d.transforms")
        assert T.quaternion_multiply.__module__ == "sgn_rast.quat"
        g = torch.Generator().manual_seed(0)
        a = torch.randn(4, generator=g, dtype=torch.float64)
        b = torch.randn(50, 4, generator=g)
        out = T.quaternion_multiply(a, b)
        assert out.dtype == torch.float32 and bool((out[:, 0] >= 0).all())
        # against rotation matrices: R(a (x) b) == R(a) R(b)
        from sgn_rast.ops import quat_to_rotmat
        Ra, Rb, Ro = quat_to_rotmat(a.float()), quat_to_rotmat(b), quat_to_rotmat(out)
        assert torch.allclose(Ro, Ra[None] @ Rb, atol=1e-5)
        i, j, k = torch.tensor([0., 1, 0, 0]), torch.tensor([0., 0, 1, 0]), torch.tensor([0., 0, 0, 1])
        assert torch.equal(T.quaternion_multiply(i, j), k)                # ij = k
        assert torch.equal(T.quaternion_multiply(j, i), -k)               # ji = -k (real part 0: sign kept)
        assert torch.equal(T.quaternion_multiply(-i, i), torch.tensor([1., 0, 0, 0]))
    finally:
        for name, mod in zip(("pytorch3d", "pytorch3d.transforms"), saved):
            sys.modules.pop(name, None)
            if mod is not None:
                sys.modules[name] = mod


def test_ply_round_trip_and_inria_field_order(tmp_path):
    from sgn_rast import io, scenes
    cam = scenes.make_camera(64, 48, 64.0)
    P = scenes.make_gaussians(500, cam, seed=3)
    P["means"][7, 1] = float("nan")                                  # dropped on export, like the reference does
    path = str(tmp_path / "point_cloud.ply")
    assert io.write_ply(path, P) == 499
    head = open(path, "rb").read(2000).split(b"end_header")[0].decode()
    props = [ln.split()[-1] for ln in head.splitlines() if ln.startswith("property")]
    assert props[:9] == ["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"]
    assert props[9] == "f_rest_0" and props[9 + 45 - 1] == "f_rest_44"                # 15 coefficients x 3 channels
    assert props[-8:] == ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    assert "format binary_little_endian 1.0" in head and "element vertex 499" in head
    Q = io.read_ply(path)
    keep = torch.arange(500) != 7
    for k in P:
        assert torch.equal(Q[k], P[k][keep]), k
    # channel-major f_rest (the INRIA order): f_rest_1 is coefficient 1 of channel 0, f_rest_15 coefficient 0 of channel 1
    import numpy as np
    raw = np.frombuffer(open(path, "rb").read().split(b"end_header\n")[1], dtype="<f4").reshape(499, -1)
    assert raw[0, 9 + 1] == float(P["features_rest"][0, 1, 0]) and raw[0, 9 + 15] == float(P["features_rest"][0, 0, 1])


def test_checkpoint_state_names_and_size_changing_load():
    from sgn_rast import io, scenes
    cam = scenes.make_camera(64, 48, 64.0)
    bg, obj = scenes.make_gaussians(300, cam, seed=1), scenes.make_gaussians(120, cam, seed=2)
    st = io.model_state({"background": bg, "object_7": obj})
    assert "all_models.background.gauss_params.scales" in st and "all_models.object_7.gauss_params.opacities" in st
    st["all_models.background.env_map.base"] = torch.zeros(6, 2, 2, 3)        # foreign keys are ignored
    back = io.load_model_state(st)
    assert set(back) == {"background", "object_7"} and back["object_7"]["means"].shape[0] == 120
    for k in bg:
        assert torch.equal(back["background"][k], bg[k]) and back["background"][k].requires_grad
    single = io.load_model_state({k: v for k, v in zip(["means", "scales", "quats", "features_dc", "features_rest",
                                                        "opacities"], [bg["means"], bg["log_scales"], bg["quats"],
                                                                       bg["features_dc"], bg["features_rest"],
                                                                       bg["opacity_logits"]])})   # old flat names
    assert torch.equal(single[""]["log_scales"], bg["log_scales"])


def test_empty_view_returns_the_reference_empty_outputs_and_still_reaches_the_reducer():
    """sgn_splatfacto.py:878-886: `radii.sum() == 0` -> background image, zero accumulation / depth.  The replay must
    return those (not raise), and `train_step` must still call `reducer.finish()` so a data-parallel rank whose view
    sees nothing joins the collectives."""
    import oracle_ops
    from sgn_rast import scenes, step
    cam = scenes.make_camera(64, 48, 64.0)
    raw = scenes.make_gaussians(200, cam, seed=0, z_range=(1.0, 4.0))
    raw["means"][:, 2] = -5.0                                    # everything behind the camera
    P = step.leaf_params(raw)
    out = step.render(P, cam, ops=oracle_ops, with_depth=True, caller_syncs=True)
    assert out.empty and out.rgb.shape == (48, 64, 3) and float(out.rgb.abs().max()) == 0.0
    assert float(out.alpha.abs().max()) == 0.0 and out.depth.shape == (48, 64, 1)

    class Reducer:
        called = 0

        def finish(self):
            Reducer.called += 1
    w_img, w_a = step.loss_weights(cam)
    res = step.train_step(P, cam, w_img, w_a, ops=oracle_ops, reducer=Reducer(), caller_syncs=True)
    assert Reducer.called == 1 and float(res.loss) == 0.0
    assert all(p.grad is None for p in P.values())


def test_graph_proofs_recognise_the_reference_expressions_on_this_torch(monkeypatch):
    """The graph proofs (`sgn_rast.proofs`) read autograd node types and saved attributes, which belong to
    the installed PyTorch, not to a documented API: pin, on CPU tensors, that the reference's expressions
    (sgn_splatfacto.py:857,858,864,940,949,988) are still recognised and that near misses are not.  (If a PyTorch
    upgrade renames a node, `proofs.enabled()` switches every proof off after its own self-test and the operators take
    their plain autograd path: correct, slower — this test is what notices.)"""
    from sgn_rast import proofs
    monkeypatch.setattr(proofs, "need_device", False)
    assert proofs.selftest() and proofs.enabled()
    n, k = 50, 16
    dc = torch.randn(n, 1, 3, requires_grad=True)
    rest = torch.randn(n, k - 1, 3, requires_grad=True)
    ls = torch.randn(n, 3, requires_grad=True)
    rq = torch.randn(n, 4, requires_grad=True)
    lo = torch.randn(n, 1, requires_grad=True)
    src = proofs.sh_source(torch.cat((dc, rest), dim=1))                      # :858
    assert src is not None and src.dc[0].leaf is dc and src.dc[0].weights is None and src.rest == (rest,)
    assert proofs.exp_leaves(torch.exp(ls)) == (ls,)                          # :857
    assert proofs.normalised_source(rq / rq.norm(dim=-1, keepdim=True)) is rq  # :864
    assert proofs.sigmoid_leaves(torch.sigmoid(lo)) == (lo,)                  # :949
    sh = torch.randn(n, 3, requires_grad=True) * 1.0
    pre = proofs.clamp_pre(torch.clamp(sh + 0.5, min=0.0))                    # :940
    assert pre is not None and type(pre.grad_fn).__name__ == "AddBackward0" and pre.shape == (n, 3)
    # near misses
    assert proofs.sh_source(torch.cat((dc, rest), dim=1) * 1.0) is None
    assert proofs.sh_source(torch.cat((dc * 1.0, rest), dim=1)) is None
    assert proofs.sh_source(torch.cat((dc, rest), dim=1).detach()) is None
    assert proofs.sh_source(torch.cat((rest, dc), dim=1)) is None
    hooked = torch.cat((dc, rest), dim=1)
    hooked.register_hook(lambda g: g)
    assert proofs.sh_source(hooked) is None
    kept = torch.cat((dc, rest), dim=1)
    kept.retain_grad()
    assert proofs.sh_source(kept) is None
    assert proofs.exp_leaves(torch.exp(ls) * 1.0) is None
    assert proofs.exp_leaves(torch.exp(ls * 1.0)) is None
    assert proofs.normalised_source(rq / rq.norm(dim=-1)[:, None]) is None
    assert proofs.normalised_source(rq / rq.norm(p=1, dim=-1, keepdim=True)) is None
    assert proofs.normalised_source(rq / (rq * 1.0).norm(dim=-1, keepdim=True)) is None
    assert proofs.sigmoid_leaves(torch.sigmoid(lo * 1.0)) is None
    assert proofs.clamp_pre(torch.clamp(sh + 0.5, min=0.0, max=1.0)) is None
    assert proofs.clamp_pre(torch.clamp(sh + 0.5, min=0.1)) is None
    written = torch.exp(ls)
    written.mul_(1.0)                                                          # modified after it was made
    assert proofs.exp_leaves(written) is None


def test_graph_proofs_follow_the_scene_graph_aggregation(monkeypatch):
    """The scene graph's parameters are row-wise concatenations over the sub-models
    (sgn_splatfacto_scene_graph.py:355-360), the objects' quaternions products with the box rotation (:416, through the
    pytorch3d shim), their DC term a Fourier sum (:239-247), and the sub-model passes receive concatenations of the
    per-model SPLITS of the main projection (:153-215, 249-276).  Every one of those shapes must be proven, and the
    windows must come out right."""
    from sgn_rast import proofs
    from sgn_rast.quat import quaternion_raw_multiply
    monkeypatch.setattr(proofs, "need_device", False)
    counts, k, F = [30, 7, 9], 16, 5
    mk = lambda *s: torch.randn(*s).requires_grad_(True)
    models = [dict(ls=mk(c, 3), rq=mk(c, 4), lo=mk(c, 1), rest=mk(c, k - 1, 3),
                   dc=mk(c, 1 if i == 0 else F, 3)) for i, c in enumerate(counts)]
    cat = lambda key: torch.concat([m[key] for m in models], dim=0)               # get_aggreated_variable :138-146
    assert proofs.exp_leaves(torch.exp(cat("ls"))) == tuple(m["ls"] for m in models)
    assert proofs.sigmoid_leaves(torch.sigmoid(cat("lo"))) == tuple(m["lo"] for m in models)
    q_o2w = torch.tensor([0.9, 0.1, -0.3, 0.2], dtype=torch.float64)
    x = torch.cat([models[0]["rq"]] + [quaternion_raw_multiply(q_o2w, m["rq"]).float() for m in models[1:]], dim=0)
    assert proofs.normalised_source(x / x.norm(dim=-1, keepdim=True)) is x       # a non-leaf X is fine
    w = [torch.randn(1, F) for _ in models]
    dcs = [models[0]["dc"]] + [torch.sum(m["dc"] * w[i][..., None], dim=1, keepdim=True)   # get_fourier_features
                               for i, m in enumerate(models) if i > 0]
    src = proofs.sh_source(torch.cat((torch.cat(dcs, dim=0), cat("rest")), dim=1))
    assert src is not None and [p.leaf for p in src.dc] == [m["dc"] for m in models]
    assert src.dc[0].weights is None and torch.equal(src.dc[2].weights, w[2][0])
    assert src.rest == tuple(m["rest"] for m in models)
    # a Fourier sum whose weights carry a gradient, or summed over another dim, is not the reference's expression
    wg = torch.randn(1, F, requires_grad=True)
    bad = torch.cat((torch.cat([dcs[0], torch.sum(models[1]["dc"] * wg[..., None], dim=1, keepdim=True), dcs[2]], 0),
                     cat("rest")), dim=1)
    assert proofs.sh_source(bad) is None
    # sub-model windows: objects = parts 1.., background = part 0
    xys = mk(sum(counts), 2) * 1.0
    parts = torch.split(xys, counts)
    sc = proofs.split_cat
    full = sc(torch.concat(parts, dim=0))
    assert full is not None and full.whole and full.rows == (0, 46)
    assert proofs.window_of_split(sc(torch.cat(parts[1:], dim=0)), full) == (30, 46)
    assert proofs.window_of_split(sc(torch.cat(parts[:1], dim=0)), full) == (0, 30)
    assert sc(torch.cat([parts[2], parts[1]], dim=0)) is None
    other = torch.split(mk(sum(counts), 2) * 1.0, counts)
    assert proofs.window_of_split(sc(torch.cat(other[1:], dim=0)), full) is None   # parts of another projection
    assert proofs.window_of_split(sc(torch.cat(parts[1:], dim=0)), sc(torch.concat(parts[:2], dim=0))) is None
    written = torch.cat(parts[1:], dim=0)
    written.add_(0.0)
    assert sc(written) is None
    leaves = [m["lo"] for m in models]
    assert proofs.window_of_leaves(leaves[1:], leaves) == (30, 46)
    assert proofs.window_of_leaves(leaves[:1], leaves) == (0, 30)
    assert proofs.window_of_leaves([leaves[2], leaves[1]], leaves) is None


def test_graph_proofs_gate_on_the_torch_version(monkeypatch, caplog):
    """An untested PyTorch series runs the matchers' self-test once; if an expression is no longer recognised every proof
    is switched off with ONE logged notice (VERDICT r03 #6b)."""
    import logging
    from sgn_rast import proofs
    monkeypatch.setattr(proofs, "_enabled", None)
    monkeypatch.setattr(proofs, "TESTED_TORCH_SERIES", ("0.0",))
    assert proofs.enabled()                                   # untested series, self-test passes: proofs stay on
    monkeypatch.setattr(proofs, "_enabled", None)
    monkeypatch.setattr(proofs, "selftest", lambda: False)
    with caplog.at_level(logging.WARNING, logger="sgn_rast.proofs"):
        assert not proofs.enabled() and not proofs.enabled()
    assert sum("not recognised" in r.message for r in caplog.records) == 1
    monkeypatch.setattr(proofs, "_enabled", None)


def test_row_exchange_counts_sub_model_passes_as_views():
    """A rasterize pass over an id range / with group accumulations reaches rows the full pass's walked list does not
    hold: the sink counts it as another view (and `_finish_sparse` then refuses the step instead of dropping rows)."""
    from types import SimpleNamespace
    from sgn_rast import dp
    r = SimpleNamespace(sparse=True, active=True, _rows_now=True, _early=dict(views=1))
    dp.GradAllReducer.extra_pass(r)
    assert r._early["views"] == 2
    r = SimpleNamespace(sparse=True, active=True, _rows_now=True, _early=None)
    dp.GradAllReducer.extra_pass(r)                       # before the step's full pass: remembered for finish()
    assert r._extra_before is True
    r = SimpleNamespace(sparse=False, active=True, _rows_now=False, _early=dict(views=1))
    dp.GradAllReducer.extra_pass(r)
    assert r._early["views"] == 1
    r = SimpleNamespace(sparse=True, active=True, _rows_now=False, _early=dict(views=1))   # a DENSE step of the adaptive
    dp.GradAllReducer.extra_pass(r)                                                         # reducer (round 6): nothing
    assert r._early["views"] == 1                                                           # is announced, nothing counted


def test_memo_remembers_pure_host_functions_by_value():
    """`fused.memo` (the scene-graph patch's per-object `quaternion_from_matrix` / `IDFT`): same function + equal
    arguments -> the remembered result, numpy arguments by their bytes, anything else a new evaluation."""
    import numpy as np
    from sgn_rast import fused
    calls = []

    def f(a, k=0):
        calls.append(1)
        return float(np.sum(a)) + k

    rot = np.arange(9.0).reshape(3, 3)
    assert fused.memo(f, rot) == 36.0 and fused.memo(f, rot.copy()) == 36.0 and len(calls) == 1
    assert fused.memo(f, rot + 1) == 45.0 and len(calls) == 2            # other bytes: evaluated
    assert fused.memo(f, rot, 2) == 38.0 and len(calls) == 3             # other scalar argument: evaluated
    assert fused.memo(f, rot, 2) == 38.0 and len(calls) == 3


def test_sort_ranking_policy_defaults_to_the_documented_form(monkeypatch):
    """Round 5: the in-wave ranking of the radix sorts is an argument of the calls; the host's default is 0 (ballot match:
    documented ISA semantics), the atomic form an opt-in that needs a GPU probe — without a GPU it stays 0 whatever the
    environment says; `force_sort_rank` overrides inside its block only."""
    from sgn_rast import _lib as L
    from sgn_rast import config
    monkeypatch.setattr(L, "_SORT_RANK", {})
    monkeypatch.setattr(L, "_sort_rank_request", "ballot")
    assert L.sort_rank_mode() == 0 and L.sort_ranking_report()["mode"] == "ballot"
    monkeypatch.setattr(L, "_sort_rank_request", None)
    with config.override(sort_rank="atomic"):                  # (the one options object: sgn_rast/config.py)
        if not torch.cuda.is_available():
            assert L.sort_rank_mode() == 0             # no device to prove it on
    with config.override(sort_rank="atomic-unchecked"):
        assert L.sort_rank_mode() == 1 and "unchecked" in L.sort_ranking_report()["probe"]
    monkeypatch.setattr(L, "_SORT_RANK", {})
    monkeypatch.setattr(L, "_sort_rank_request", "ballot")
    with L.force_sort_rank("atomic"):
        assert L.sort_rank_mode() == 1
        with L.force_sort_rank("ballot"):
            assert L.sort_rank_mode() == 0
        assert L.sort_rank_mode() == 1
    assert L.sort_rank_mode() == 0


def test_densification_statistics_bookkeeping_without_a_process_group():
    """`Stats` outside torch.distributed: the reference's single-process arithmetic (first update counts every Gaussian
    once), `sync` is a no-op that says whether there is anything to decide on, `reset` forgets the interval."""
    from helpers import TorchStats
    S = TorchStats()
    assert S.sync() is False
    g = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0]])
    r = torch.tensor([5, 0, 2], dtype=torch.int32)
    S.update(g, r, (10, 20), step=7)
    assert torch.equal(S.vis_counts, torch.ones(3)) and torch.equal(S.xys_grad_norm, torch.tensor([5.0, 0.0, 1.0]))
    assert torch.equal(S.max_2Dsize, torch.tensor([0.25, 0.0, 0.1])) and S._first_key is None
    S.update(g, r, (10, 20), step=8)
    assert torch.equal(S.vis_counts, torch.tensor([2.0, 1.0, 2.0])) and S.sync() is True and S.synced_dim is None
    S.reset()
    assert S.xys_grad_norm is None and S.sync() is False


@pytest.mark.parametrize("parts", [(1, 1, 0), (0, 0, 1), (1, 1, 1)], ids=["xys+depths", "conics", "all"])
def test_viewmat_gradient_assembly_from_the_backward_kernels_outputs(torch_oracle, c_oracle, parts):
    """`ops._viewmat_grad` turns the per-Gaussian `v_mean` / `v_cov2d` of the projection backward into dL/d(viewmat).
    Here the C oracle's backward supplies those two (same formulas as the HIP kernel, test_gpu_parity) and fp64 autograd
    through the pure-PyTorch oracle is the answer; tests/test_gpu_parity.py repeats it through the HIP node."""
    import math
    from helpers import activated, rel_l2, small_scene
    cam, P = small_scene(n=4000)
    scales, quats, _, _ = activated(P)
    means, n = P["means"], P["means"].shape[0]
    c, s = math.cos(0.07), math.sin(0.07)
    V = torch.eye(4)
    V[:3] = cam.viewmat[:3]
    V = (torch.tensor([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]]) @ V)[:3].contiguous()
    g = torch.Generator().manual_seed(4)
    w_xy, w_d, w_c = torch.randn(n, 2, generator=g), torch.randn(n, generator=g), torch.randn(n, 3, generator=g)
    intr = (cam.fx, cam.fy, cam.cx, cam.cy, cam.height, cam.width, 16)
    vm = V.double().clone().requires_grad_(True)
    out = torch_oracle.project_gaussians(means.double(), scales.double(), 1.0, quats.double(), vm, *intr)
    live = out[2] > 0
    (parts[0] * (out[0] * w_xy.double())[live].sum() + parts[1] * (out[1] * w_d.double())[live].sum()
     + parts[2] * (out[3] * w_c.double())[live].sum()).backward()
    xys, depths, radii, conics, comp, nth, cov3d = c_oracle.project_fwd(means, scales, 1.0, quats, V, *intr)
    assert torch.equal(radii > 0, live)
    m = (radii > 0).float()
    v_mean, _, _, v_cov2d, _ = c_oracle.project_bwd(means, scales, 1.0, quats, V, cam.fx, cam.fy, cov3d, radii, conics,
                                                    comp, parts[0] * w_xy * m[:, None], parts[1] * w_d * m,
                                                    parts[2] * w_c * m[:, None], torch.zeros(n))
    for shape in ((3, 4), (4, 4)):
        got = ops._viewmat_grad(means, V.reshape(-1), cam.fx, cam.fy, cov3d, radii, v_mean, v_cov2d, shape)
        assert tuple(got.shape) == shape and got.dtype == torch.float32
        assert rel_l2(got[:3].double(), vm.grad) < 1e-5
        assert float(got[3:].abs().sum()) == 0.0


def test_one_options_object_and_one_environment_variable():
    """Round 6: every behaviour switch is a row of `sgn_rast.config.OPTIONS`, initialised from ONE
    environment variable, `SGN_OPTIONS="name=value,..."`; unknown names / values raise; no other SGN_* variable
    configures behaviour (three deployment variables of the launcher excepted, as the module says)."""
    import os
    import re
    import subprocess
    import sys
    from sgn_rast import config
    assert config._convert("quat_check", "Deferred") == "deferred" and config._convert("graph_proofs", "off") is False
    assert config._convert("batch_fwd", "64") == 64 and config._convert("reduce_mode", "0") == 0
    with pytest.raises(ValueError):
        config._convert("quat_check", "sometimes")
    with pytest.raises(ValueError):
        config._convert("reduce_mode", "2")                # the MFMA reduction is gone
    pkg = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "street-gaussians-ns_amd")
    env = dict(os.environ, SGN_OPTIONS="quat_check=deferred, one_call_nodes=off,batch_fwd=64", PYTHONPATH=pkg)
    out = subprocess.check_output([sys.executable, "-c",
                                   "from sgn_rast import ops, config; print(ops.quat_check, ops.composite_forward, "
                                   "ops.composite_backward, config.value('batch_fwd'), ops.depth_channel)"], env=env, text=True)
    assert out.split() == ["deferred", "False", "False", "64", "auto"]
    bad = subprocess.run([sys.executable, "-c", "import sgn_rast"], env=dict(env, SGN_OPTIONS="quat_chek=off"),
                         capture_output=True, text=True)
    assert bad.returncode != 0 and "unknown option" in bad.stderr
    # no module of the package reads another SGN_* variable for behaviour
    allowed = {"SGN_OPTIONS", "SGN_RAST_LIB", "SGN_DP_BACKEND", "SGN_DP_TIMEOUT_S"}
    for fn in os.listdir(os.path.join(pkg, "sgn_rast")):
        if fn.endswith(".py") and fn != "config.py":
            txt = open(os.path.join(pkg, "sgn_rast", fn)).read()
            for m in re.finditer(r"environ[^\n]*?[\"'](SGN_[A-Z0-9_]+)[\"']", txt):
                assert m.group(1) in allowed, (fn, m.group(1))
    for name, (default, allowed_v, targets, doc) in config.OPTIONS.items():
        assert targets and doc and (allowed_v is int or default in allowed_v), name
