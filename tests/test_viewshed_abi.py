"""The host half of the viewshed (include/atmrt.h): names and the struct size, atmrt_viewshed_fan_angles against the numpy expression
bit for bit (at K = 64 also against atmrt_sight_fan_angles), the kernel's shape, and NULL contexts.  The library loads without a GPU;
nothing here touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import viewshed_model as vm
from atm_raytracer_amd import _abi, _lib, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_viewshed", "atmrt_viewshed_device", "atmrt_viewshed_fan_angles", "atmrt_debug_viewshed_shape", "atmrt_viewshed_steps",
         "atmrt_last_viewshed_timings", "atmrt_last_viewshed_work")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_names_and_struct_size(lib):
    header = open(os.path.join(ROOT, "include", "atmrt.h")).read()
    declared = set(re.findall(r"\b(atmrt_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.atmrt_abi_sizeof(28) == C.sizeof(_abi.ViewshedSpec) == 56
    assert lib.atmrt_abi_sizeof(27) == 0 and lib.atmrt_abi_sizeof(29) == 0 and lib.atmrt_abi_version() == 5
    assert [n for n, _ in _abi.ViewshedSpec._fields_] == ["az_lo_deg", "az_step_deg", "reach", "height", "fan_lo_deg", "fan_hi_deg", "n_az", "fan_rays"]
    assert _abi.ViewshedSpec.n_az.offset == 48 and _abi.ViewshedSpec.fan_rays.offset == 52
    assert "viewshed" in header and "first round of the sight-line rule" in header.lower().replace("\n * ", " ")
    assert [k for k, _ in generators.VIEWSHED_PLANES] == [k for k, _ in vm.PLANES] and [np.dtype(t) for _, t in generators.VIEWSHED_PLANES] == [np.dtype(t) for _, t in vm.PLANES]


FANS = [(-5.0, 5.0), (-1.0, 1.0), (0.0, 1.0), (-0.3, 2.9), (1e-3, 1e-3 + 1e-9), (-90.0, 90.0), (0.25, np.nextafter(0.25, 1.0)), (-2.0 / 3.0, 2.0 / 3.0)]


@pytest.mark.parametrize("K", [64, 128, 576, 1024, 4096])
def test_fan_angles_equal_the_numpy_expression(lib, K):
    for lo, hi in FANS:
        got = generators.viewshed_fan_angles(lo, hi, K, lib)
        want = lo + np.arange(K, dtype=np.float64) * ((hi - lo) / np.float64(K - 1))
        assert got.shape == (K,) and got.tobytes() == want.tobytes() == vm.fan_angles(lo, hi, K).tobytes(), (lo, hi, K, np.flatnonzero(got != want)[:5])
        assert got[0] == lo and (np.diff(got) >= 0).all()
        if K == 64:
            assert got.tobytes() == generators.sight_fan_angles(lo, hi, lib).tobytes(), (lo, hi)


def test_fan_angles_random_fans_equal_the_sight_lines_at_64(lib):
    rng = np.random.default_rng(28)
    for _ in range(500):
        lo = float(rng.uniform(-10, 10))
        hi = lo + float(10.0 ** rng.uniform(-14, 1.5))
        got = generators.viewshed_fan_angles(lo, hi, 64, lib)
        assert got.tobytes() == generators.sight_fan_angles(lo, hi, lib).tobytes() == vm.fan_angles(lo, hi, 64).tobytes(), (lo, hi)
        K = 64 * int(rng.integers(1, 65))
        assert generators.viewshed_fan_angles(lo, hi, K, lib).tobytes() == vm.fan_angles(lo, hi, K).tobytes(), (lo, hi, K)


def test_fan_angles_refuse_bad_arguments(lib):
    out = np.full(4200, -7.0)
    for K in (0, -64, 1, 63, 65, 100, 4097, 4160, 1 << 20):
        assert lib.atmrt_viewshed_fan_angles(-1.0, 1.0, K, out.ctypes.data) == _abi.ERR_INVALID_ARGUMENT, K
    assert lib.atmrt_viewshed_fan_angles(-1.0, 1.0, 64, None) == _abi.ERR_INVALID_ARGUMENT
    for lo, hi in ((np.nan, 1.0), (-1.0, np.inf), (-np.inf, np.nan)):
        assert lib.atmrt_viewshed_fan_angles(lo, hi, 64, out.ctypes.data) == _abi.ERR_INVALID_ARGUMENT
    assert (out == -7.0).all()  # a refused call writes nothing
    assert lib.atmrt_viewshed_fan_angles(-1.0, 1.0, 4096, out.ctypes.data) == 0 and out[4095] != -7.0 and out[4096] == -7.0


def test_kernel_shape(lib):
    s64 = generators.viewshed_kernel_shape(64, lib)
    assert s64["az_per_load"] >= 2 and s64["step_tile"] >= 2 and s64["rays_per_lane"] == 1
    per_lane = [generators.viewshed_kernel_shape(K, lib)["rays_per_lane"] for K in range(64, 4097, 64)]
    assert per_lane[-1] >= 2 and all(a <= b for a, b in zip(per_lane, per_lane[1:]))  # never fewer rays per lane for a larger fan
    assert generators.viewshed_kernel_shape(100, lib)["rays_per_lane"] == 0 and generators.viewshed_kernel_shape(4160, lib)["rays_per_lane"] == 0
    assert lib.atmrt_debug_viewshed_shape(64, None, None, None) == 0
    # every variant of the scan kernel (every distinct number of rays per lane over the fans the call accepts) is among the fans
    # tests/test_gpu_viewshed.py runs: a new variant cannot go untested
    fans = vm.gpu_fan_rays(lambda K: generators.viewshed_kernel_shape(K, lib)["rays_per_lane"])
    assert {generators.viewshed_kernel_shape(K, lib)["rays_per_lane"] for K in fans} == set(per_lane) and 0 not in per_lane
    assert {64, 128, 4096} <= set(fans) and len(fans) <= 8


def test_null_context(lib):
    spec = _abi.ViewshedSpec(0.0, 1.0, 1_000.0, 0.0, -1.0, 1.0, 1, 64)
    k, st, hid = np.zeros(16, np.uint16), np.zeros(16, np.uint8), np.zeros(16)
    for fn in (lib.atmrt_viewshed, lib.atmrt_viewshed_device):
        assert fn(None, C.byref(spec), k.ctypes.data, st.ctypes.data, hid.ctypes.data, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_viewshed_steps(None, 1_000.0, C.byref(C.c_int32())) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_last_viewshed_timings(None, (C.c_double * 4)()) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_last_viewshed_work(None, C.byref(C.c_int32()), C.byref(C.c_int32())) == _abi.ERR_INVALID_ARGUMENT
