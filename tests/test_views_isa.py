"""CPU, compile only: the batched-views kernels keep their state in registers / LDS (ScratchSize 0), the view-aware raster
kernels keep reading the 48-byte rows into SGPRs (s_load_dwordx8), and the projection / SH / opacity sums over the
views use no float atomics."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "street-gaussians-ns_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _asm(tmp_path_factory, name):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found")
    d = tmp_path_factory.mktemp(f"views_isa_{name}")
    extra = ["-fno-slp-vectorize"] if name == "raster" else []      # as csrc/Makefile builds it
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *extra, "--cuda-device-only", "-S", "-o",
           str(d / f"{name}.s"), os.path.join(CSRC, f"{name}.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=900, cwd=d)
    return open(d / f"{name}.s").read()


def _kernels(asm):
    return {m.group(1): m.group(0) for m in
            re.finditer(r"^(_Z\w+):.*?s_endpgm(.*?)(?=^_Z\w+:|\Z)", asm, re.S | re.M)}


EXPECTED = {"project": (["project_views_fwd_kernel", "project_views_bwd_kernel"], 2),
            "sh": (["sh_views_fwd_kernel", "sh_views_bwd_kernel"], 10),
            "binning": (["bin_emit_views_kernel"], 2),
            "raster": (["raster_views_fwd_kernel", "raster_views_bwd_kernel", "raster_views_bwd_short_kernel",
                        "unpack_views_kernel", "views_repeat_kernel"], 4 + 4 + 4 + 1 + 1)}


@pytest.mark.parametrize("tu", sorted(EXPECTED))
def test_views_kernels_have_no_scratch(tmp_path_factory, tu):
    ks = _kernels(_asm(tmp_path_factory, tu))
    names, count = EXPECTED[tu]
    mine = {k: t for k, t in ks.items() if any(n in k for n in names)}
    assert len(mine) == count, sorted(mine)
    for k, t in mine.items():
        assert re.search(r"ScratchSize: 0\b", t), f"{k} uses scratch"
        if tu in ("project", "sh") or "unpack_views" in k:
            assert "global_atomic_add_f32" not in t and "global_atomic_pk_add" not in t, k
        if "raster_views" in k:
            assert "s_load_dwordx8" in t, k      # the 48-byte rows stay on the scalar path
    if tu == "raster":
        # the existing kernels' names stay countable by test_isa_properties' substrings
        for legacy in ("raster_fwd_kernel", "raster_fwd_pk_kernel", "raster_bwd_kernel", "raster_bwd_short_kernel"):
            assert not any(legacy in k for k in mine), legacy
