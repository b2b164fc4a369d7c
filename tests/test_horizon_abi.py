"""The host half of the horizon (include/atmrt.h): names, struct sizes and layouts, the scan's shape, and NULL contexts.  The library
loads without a GPU; nothing here touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import horizon_model as hm
import viewshed_model as vm
from atm_raytracer_amd import _abi, _lib, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_horizon", "atmrt_horizon_device", "atmrt_debug_horizon_shape", "atmrt_last_horizon_timings", "atmrt_last_horizon_work")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_names_and_struct_sizes(lib):
    header = open(os.path.join(ROOT, "include", "atmrt.h")).read()
    declared = set(re.findall(r"\b(atmrt_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.atmrt_abi_sizeof(30) == C.sizeof(_abi.HorizonSpec) == 56
    assert lib.atmrt_abi_sizeof(31) == C.sizeof(_abi.Horizon) == 72
    assert lib.atmrt_abi_sizeof(29) == 0 and lib.atmrt_abi_sizeof(32) == 0 and lib.atmrt_abi_version() == 5
    for gap in (17, 23, 27):
        assert lib.atmrt_abi_sizeof(gap) == 0, gap
    assert [n for n, _ in _abi.HorizonSpec._fields_] == ["az_lo_deg", "az_step_deg", "reach", "fan_lo_deg", "fan_hi_deg", "n_az", "fan_rays", "rounds"]
    assert (_abi.HorizonSpec.n_az.offset, _abi.HorizonSpec.fan_rays.offset, _abi.HorizonSpec.rounds.offset) == (40, 44, 48)
    assert "horizon" in header and "atmrt_horizon_spec_t" in header and "atmrt_horizon_t" in header


def test_dtypes():
    assert generators.HORIZON_DTYPE == hm.HORIZON_DTYPE and generators.HORIZON_DTYPE.itemsize == C.sizeof(_abi.Horizon) == 72
    assert [n for n, _ in _abi.Horizon._fields_] == list(generators.HORIZON_DTYPE.names)
    for name in generators.HORIZON_DTYPE.names:
        assert generators.HORIZON_DTYPE.fields[name][1] == getattr(_abi.Horizon, name).offset, name
    assert (_abi.HORIZON_FOUND, _abi.HORIZON_ABOVE_FAN, _abi.HORIZON_BELOW_FAN) == (hm.FOUND, hm.ABOVE_FAN, hm.BELOW_FAN) == (0, 2, 3)
    assert (_abi.HORIZON_ABOVE_FAN, _abi.HORIZON_BELOW_FAN) == (_abi.SIGHT_ABOVE_FAN, _abi.SIGHT_BELOW_FAN)
    assert generators.HORIZON_COLUMNS == ("azimuth_deg", "status", "angle_clear_deg", "angle_blocked_deg", "resolution_deg", "ridge_distance_m", "ridge_lat",
                                          "ridge_lon", "ridge_elevation_m")


def test_kernel_shape(lib):
    s64 = generators.horizon_kernel_shape(64, lib)
    assert s64["az_per_load"] >= 2 and s64["step_tile"] >= 2 and s64["rays_per_lane"] == 1
    per_lane = [generators.horizon_kernel_shape(K, lib)["rays_per_lane"] for K in range(64, 4097, 64)]
    assert per_lane[-1] >= 2 and all(a <= b for a, b in zip(per_lane, per_lane[1:])) and 0 not in per_lane
    assert generators.horizon_kernel_shape(100, lib)["rays_per_lane"] == 0 and generators.horizon_kernel_shape(4160, lib)["rays_per_lane"] == 0
    assert lib.atmrt_debug_horizon_shape(64, None, None, None) == 0
    # every variant of the scan kernel is among the fans tests/test_gpu_horizon.py runs: a new variant cannot go untested
    fans = vm.gpu_fan_rays(lambda K: generators.horizon_kernel_shape(K, lib)["rays_per_lane"])
    assert {generators.horizon_kernel_shape(K, lib)["rays_per_lane"] for K in fans} == set(per_lane)
    assert {64, 128, 4096} <= set(fans) and len(fans) <= 8


def test_csv(tmp_path):
    rec = np.zeros(2, dtype=generators.HORIZON_DTYPE)
    rec[0] = (0, 3, 40, 17, 1.25, 1.0, 0.25, 1700.0, 46.5, 8.75, 812.5)
    rec[1] = (2, 1, 64, -1, np.nan, 5.0, 0.125, np.nan, np.nan, np.nan, np.nan)
    generators.write_horizon_csv(str(tmp_path / "h.csv"), generators.Horizon(rec, np.array([10.0, 10.5]), np.zeros(64)))
    assert (tmp_path / "h.csv").read_text().splitlines() == [",".join(generators.HORIZON_COLUMNS), "10.0,found,1.25,1.0,0.25,1700.0,46.5,8.75,812.5",
                                                            "10.5,above_fan,,5.0,0.125,,,,"]


def test_null_context(lib):
    spec = _abi.HorizonSpec(0.0, 1.0, 1_000.0, -1.0, 1.0, 1, 64, 3)
    out = np.zeros(1, dtype=generators.HORIZON_DTYPE)
    for fn in (lib.atmrt_horizon, lib.atmrt_horizon_device):
        assert fn(None, C.byref(spec), out.ctypes.data) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_last_horizon_timings(None, (C.c_double * 5)()) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_last_horizon_work(None, C.byref(C.c_int32()), C.byref(C.c_int32())) == _abi.ERR_INVALID_ARGUMENT
