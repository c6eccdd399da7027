"""CPU, compile only: every kernel of csrc/cloud_nn.hip (the shared tree build and the two-cloud query) keeps its state
in registers / LDS (ScratchSize 0: one register best, the traversal stack in LDS) and the query kernel reads a leaf's
candidates through scalar loads."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "street-gaussians-ns_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def cloud_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.fail("hipcc not found")
    d = tmp_path_factory.mktemp("cloud_nn_isa")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-munsafe-fp-atomics",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "--save-temps", "-c", "-o", str(d / "cloud_nn.o"),
           os.path.join(CSRC, "cloud_nn.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600, cwd=d)
    asm = [f for f in os.listdir(d) if f.endswith(".s") and "gfx950" in f]
    assert asm, os.listdir(d)
    return open(os.path.join(d, asm[0])).read()


def _kernels(asm):
    return {m.group(1): m.group(0) for m in
            re.finditer(r"^(_Z\w+):.*?s_endpgm(.*?)(?=^_Z\w+:|\Z)", asm, re.S | re.M)}


def test_every_cloud_nn_kernel_has_no_scratch(cloud_asm):
    ks = _kernels(cloud_asm)
    for nm in ["knn_bbox_partial", "knn_morton", "knn_gather", "knn_leaf_box", "knn_level_box", "cloud_nn_query",
               "cloud_nn_query_sparse"]:
        assert any(nm in k for k in ks), nm
    assert not any("knn_query" in k for k in ks)         # tests/test_knn_isa.py counts those in knn.hip alone
    for name, text in ks.items():
        assert re.search(r"ScratchSize: 0\b", text), f"{name} uses scratch"


def test_query_kernel_reads_candidates_through_scalar_loads(cloud_asm):
    ks = _kernels(cloud_asm)
    (name,) = [k for k in ks if "cloud_nn_query" in k and "sparse" not in k]
    body = ks[name]
    assert "s_load_dwordx4" in body                                   # wave-uniform loads
    # the candidates are float4s at wave-uniform addresses: wide scalar loads from a computed base (the compiler may
    # pair two candidates into one dwordx8), and no vector load wider than a query's own xyz
    wide = re.findall(r"s_load_dwordx(?:4|8|16) s\[\d+:\d+\], s\[(\d+):\d+\], 0x[0-9a-f]+", body)
    assert len(wide) >= 6, wide
    assert not re.search(r"(?:global|flat|buffer)_load_dwordx4", body)
    assert len(re.findall(r"(?:global|flat)_load_", body)) <= 4       # the query's id and xyz, the result's id
    # the seed search probes the target's sorted keys with scalar 8-byte loads
    assert "s_load_dwordx2" in body
    # one atomic only: the optional visited sum
    assert len(re.findall(r"global_atomic_\w+", body)) == 1 and "global_atomic_add_x2" in body


def test_sparse_query_kernel_keeps_the_walk_scalar(cloud_asm):
    """One wave per query: a leaf's candidates come one per lane (a single vector load in the scan), the seed search
    and the boxes through scalar loads, and the only atomic is the visited sum."""
    ks = _kernels(cloud_asm)
    (name,) = [k for k in ks if "cloud_nn_query_sparse" in k]
    body = ks[name]
    assert "s_load_dwordx2" in body and "s_load_dwordx8" in body      # sorted keys; a node's two corners
    assert len(re.findall(r"(?:global|flat)_load_", body)) <= 3       # the query, a leaf's candidates, the result's id
    assert len(re.findall(r"global_atomic_\w+", body)) == 1 and "global_atomic_add_x2" in body
