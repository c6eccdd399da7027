"""CPU, compile only: every kernel of csrc/knn.hip keeps its state in registers / LDS (ScratchSize 0: the top-k lists
are indexed statically, the traversal stack lives in LDS) and a leaf's candidates come through scalar loads."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "street-gaussians-ns_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def knn_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found")
    d = tmp_path_factory.mktemp("knn_isa")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--save-temps", "-c", "-o", str(d / "knn.o"),
           os.path.join(CSRC, "knn.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600, cwd=d)
    asm = [f for f in os.listdir(d) if f.endswith(".s") and "gfx950" in f]
    assert asm, os.listdir(d)
    return open(os.path.join(d, asm[0])).read()


def _kernels(asm):
    return {m.group(1): m.group(0) for m in
            re.finditer(r"^(_Z\w+):.*?s_endpgm(.*?)(?=^_Z\w+:|\Z)", asm, re.S | re.M)}


def test_every_knn_kernel_has_no_scratch(knn_asm):
    ks = _kernels(knn_asm)
    names = ["knn_bbox_partial", "knn_morton", "knn_gather", "knn_leaf_box", "knn_level_box"]
    for nm in names:
        assert any(nm in k for k in ks), nm
    queries = [k for k in ks if "knn_query" in k]
    assert len(queries) == 5                                         # K buckets 1, 2, 4, 8, 16
    for name, text in ks.items():
        assert re.search(r"ScratchSize: 0\b", text), f"{name} uses scratch"
    for name in queries:
        assert "s_load_dwordx4" in ks[name]                          # wave-uniform candidate loads
