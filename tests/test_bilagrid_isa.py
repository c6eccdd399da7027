"""Compile-only checks of csrc/bilagrid.hip (hipcc cross-compiles without a GPU), built with the Makefile's common flags:
every kernel keeps everything in registers, the streaming kernels read the cells 16 bytes at a time and do nothing else, and
the gather's only adds to memory are native global float atomics — one per coefficient and workgroup, after the sums in
registers and across the waves through LDS — with no compare-and-swap loop and no LDS atomic."""
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
    out = tmp_path_factory.mktemp("isa") / "bilagrid.s"
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-S", "--cuda-device-only", "-o", str(out),
           os.path.join(CSRC, "bilagrid.hip")]
    subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    asm = out.read_text()
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_Z\w+):.*?s_endpgm(.*?)(?=^_Z\w+:|\Z)", asm, re.S | re.M)}


def test_makefile_lists_it_with_the_common_flags():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert "bilagrid.hip" in mk.split("SRCS")[1].split("\n")[0]
    assert not re.search(r"^bilagrid\.o:", mk, re.M)               # no rule of its own: the pattern rule, $(FLAGS)
    flags = re.search(r"^FLAGS\s*:=(.*\\\n)*.*$", mk, re.M).group(0)
    assert "-ffp-contract=off" in flags and "-munsafe-fp-atomics" in flags


def test_every_kernel_stays_in_registers(kernels):
    fwd = [t for k, t in kernels.items() if "bilagrid_slice_fwd_kernel" in k]
    rgb = [t for k, t in kernels.items() if "bilagrid_slice_bwd_rgb_kernel" in k]
    gather = {k: t for k, t in kernels.items() if "bilagrid_slice_bwd_grid_kernel" in k}
    # the forward, its twin for v_rgb, and the gather for 1, 4 and 8 z-levels in registers
    assert len(kernels) == 5 and len(fwd) == 1 and len(rgb) == 1 and len(gather) == 3, sorted(kernels)
    for k, t in kernels.items():
        assert re.search(r"ScratchSize: 0\b", t), f"{k} spills to scratch"
        assert "v_mfma" not in t, k
    for t in fwd + rgb:
        assert "global_load_dwordx4" in t                           # a cell row per load
        assert "atomic" not in t and not re.search(r"\bds_", t)      # they only stream


def test_backward_adds_are_native_float_atomics(kernels):
    gather = {k: t for k, t in kernels.items() if "bilagrid_slice_bwd_grid_kernel" in k}
    for k, t in gather.items():
        assert "cmpswap" not in t, k                                # no compare-and-swap loop anywhere
        assert "flat_atomic" not in t, k                            # the address space of the add is known
        assert t.count("global_atomic_add_f32") == 1, k             # one add per coefficient and workgroup, after the sums
        assert "ds_add" not in t, k                                 # nothing is summed by LDS atomics
        # the waves' partial sums meet in LDS: plain stores, a barrier, plain reads in wave order
        assert re.search(r"\bds_write", t) and re.search(r"\bds_read", t) and "s_barrier" in t, k
        assert re.search(r"v_(pk_)?fma(c)?_f32", t), k              # the running sums are the spelled fmaf
    occ = {int(re.search(r"ILi(\d+)E", k).group(1)): int(re.search(r"; Occupancy: (\d+)", t).group(1))
           for k, t in gather.items()}
    assert set(occ) == {1, 4, 8} and occ[8] >= 3, occ               # 96 sums per lane still leave three waves per SIMD
