"""CPU, compile only: the pose-gradient kernels of csrc/project.hip keep their state in registers / LDS (ScratchSize 0:
the cascade's levels are indexed statically) and reduce without float atomics (per-wave partials, fixed-order sums)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "street-gaussians-ns_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def project_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found")
    d = tmp_path_factory.mktemp("pose_isa")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--save-temps", "-c", "-o", str(d / "project.o"),
           os.path.join(CSRC, "project.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600, cwd=d)
    asm = [f for f in os.listdir(d) if f.endswith(".s") and "gfx950" in f]
    assert asm, os.listdir(d)
    return open(os.path.join(d, asm[0])).read()


def _kernels(asm):
    return {m.group(1): m.group(0) for m in
            re.finditer(r"^(_Z\w+):.*?s_endpgm(.*?)(?=^_Z\w+:|\Z)", asm, re.S | re.M)}


def test_pose_kernels_have_no_scratch_and_no_float_atomics(project_asm):
    ks = _kernels(project_asm)
    pose = [k for k in ks if "project_bwd_kernelILi1ELb1E" in k or "pose_sum_kernel" in k or "pose_final_kernel" in k]
    assert len(pose) == 3, list(ks)
    for name in pose:
        assert re.search(r"ScratchSize: 0\b", ks[name]), f"{name} uses scratch"
        assert "global_atomic_add_f32" not in ks[name] and "global_atomic_pk_add" not in ks[name], name
    assert "ds_bpermute_b32" in ks[[k for k in pose if "project_bwd" in k][0]]      # the wave scan's shuffles
