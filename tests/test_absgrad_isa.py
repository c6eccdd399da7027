"""Compile-only checks of csrc/raster_absgrad.hip (hipcc cross-compiles without a GPU), built with raster.hip's flags: the
three launch shapes of the backward, each exact x reduce, keep raster.hip's properties — rows in SGPRs, nothing in
scratch, the short-walk kernel at four waves per SIMD, no SLP-packed FP32 — and the two absolute sums cost ONE more
swap per reduction (the spare rows of the third folded register), nothing in the butterfly form's swap count."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "street-gaussians-ns_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "raster_absgrad.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
           "-fno-slp-vectorize", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-o",
           str(out), os.path.join(CSRC, "raster_absgrad.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    assert "v_mfma" not in asm
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_Z\w+):.*?s_endpgm(.*?)(?=^_Z\w+:|\Z)", asm, re.S | re.M)}


def test_makefile_builds_it_with_rasters_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "raster_absgrad.hip" in mk.split("SRCS")[1].split("\n")[0]
    rule = lambda name: re.search(r"^%s\.o:.*\n\t(.*)$" % name, mk, re.M).group(1).replace(name, "X")
    assert rule("raster_absgrad") == rule("raster") and "-fno-slp-vectorize" in rule("raster")
    assert "-ffp-contract=off" in re.search(r"^FLAGS\s*:=(.*\\\n)*.*$", mk, re.M).group(0)


def test_absgrad_backward_kernels(kernels):
    bwd = {k: t for k, t in kernels.items() if "raster_absbwd" in k}
    short = {k: t for k, t in bwd.items() if "raster_absbwd_short_kernel" in k}
    # exact (2) x reduce (2) x {in-kernel adaptive split, long-walk half, short-walk half}
    assert len(bwd) == 12 and len(short) == 4
    assert sum("Li4ELb1ELi0E" in k for k in bwd) == 4
    assert sum("Li1ELb0ELi2E" in k for k in bwd) == 4
    for k, t in bwd.items():
        assert re.search(r"ScratchSize: 0\b", t), f"{k} spills to scratch"
        assert "s_load_dwordx8" in t and "s_load_dwordx4" in t          # the 48-byte row in SGPRs
        assert "v_pk_fma_f32" not in t and "v_pk_mul_f32" not in t, k
        assert "v_mfma" not in t
        reduce_mode = int(re.search(r"raster_absbwd_(?:short_)?kernelILb[01]ELi([01])E", k).group(1))
        swaps = t.count("v_permlane32_swap") + t.count("v_permlane16_swap")
        # swap form: 9 swaps per code path (scalar chase, LDS batches) — the plain kernels' 8 and one more; butterfly: none
        assert swaps == (18 if reduce_mode == 1 else 0), (k, swaps)
        assert "global_atomic_add_f32" in t
    for k, t in short.items():
        m = re.search(r"; Occupancy: (\d+)", t)
        assert m and int(m.group(1)) == 4, (k, m and m.group(1))


def test_raster_hip_gained_no_absgrad_code():
    src = open(os.path.join(CSRC, "raster.hip")).read()
    assert "absbwd" not in src and "ABSGRAD" not in src
