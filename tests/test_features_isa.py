"""Compile-only checks (hipcc cross-compiles without a GPU) of what csrc/raster_features.hip's design relies on: no
instantiation spills to scratch, a visited entry's geometry row and features arrive through scalar loads (uniform
operands, no LDS), the backward reduces with the permlane swaps and adds a (tile, Gaussian)'s sums with ONE atomic
instruction, and the 16-channel forward stays inside the four-waves-per-SIMD register budget."""
import os
import re

import pytest

import test_isa_properties as TI
from sgn_rast import features as F  # noqa: F401  (the module whose kernels these are: without it nothing here runs)


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    if not os.path.exists(TI.HIPCC):
        pytest.skip("hipcc not available")
    out = tmp_path_factory.mktemp("isa") / "raster_features.s"
    cmd = [TI.HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-munsafe-fp-atomics",
           "-fno-slp-vectorize", "-I" + os.path.join(TI.ROOT, "include"), "-I" + TI.CSRC, "-S", "--cuda-device-only",
           "-o", str(out), os.path.join(TI.CSRC, "raster_features.hip")]                 # as csrc/Makefile builds it
    TI.subprocess.run(cmd, check=True, capture_output=True, timeout=600)
    return TI._kernels(out.read_text())


def _num(text, key):
    return int(re.search(rf"; {key}: (\d+)", text).group(1))


def test_feature_kernels_have_no_scratch_no_lds_and_scalar_operands(kernels):
    fwd = {k: t for k, t in kernels.items() if "feat_fwd_kernel" in k}
    bwd = {k: t for k, t in kernels.items() if "feat_bwd_kernel" in k}
    assert len(fwd) == 10 and len(bwd) == 10          # exact x chunk widths 1, 2, 4, 8, 16
    for k, t in {**fwd, **bwd}.items():
        assert _num(t, "ScratchSize") == 0, f"{k} spills to scratch"
        assert "s_load_dwordx8" in t, k               # the 32-byte geometry row in SGPRs
        assert "ds_read" not in t and "ds_write" not in t, k
    for k, t in fwd.items():
        if "Li16E" in k:
            assert "s_load_dwordx16" in t, k          # a full chunk's features: one wide scalar load
            assert _num(t, "NumVgprs") <= 128 and _num(t, "Occupancy") >= 4, k


def test_feature_backward_reduces_in_the_wave_and_adds_once(kernels):
    for k, t in kernels.items():
        if "feat_bwd_kernel" not in k:
            continue
        assert "v_permlane32_swap" in t and "v_permlane16_swap" in t, k
        assert len(re.findall(r"global_atomic_add_f32", t)) == 1, k
