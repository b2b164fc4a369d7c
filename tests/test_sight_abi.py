"""The host half of the sight lines (include/atmrt.h): names and struct sizes, atmrt_sight_fan_angles against the numpy expression
bit for bit, atmrt_sight_pick against the model, and the CSV tables of the command line.  The library loads without a GPU; nothing
here touches a device."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import sight_model as sm
from atm_raytracer_amd import _abi, _lib, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_sight_lines", "atmrt_sight_fan_probe", "atmrt_sight_fan_angles", "atmrt_sight_pick", "atmrt_last_sight_timings",
         "atmrt_last_sight_batches")


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
    assert lib.atmrt_abi_sizeof(24) == C.sizeof(_abi.SightTarget) == generators.SIGHT_TARGET_DTYPE.itemsize == 24
    assert lib.atmrt_abi_sizeof(25) == C.sizeof(_abi.Sight) == generators.SIGHT_DTYPE.itemsize == sm.SIGHT_DTYPE.itemsize == 88
    assert lib.atmrt_abi_sizeof(26) == C.sizeof(_abi.SightRay) == generators.SIGHT_RAY_DTYPE.itemsize == sm.RAY_DTYPE.itemsize == 24
    assert lib.atmrt_abi_sizeof(17) == 0 and lib.atmrt_abi_sizeof(23) == 0 and lib.atmrt_abi_sizeof(27) == 0
    assert lib.atmrt_abi_version() == 5
    assert generators.SIGHT_DTYPE == sm.SIGHT_DTYPE and generators.SIGHT_RAY_DTYPE == sm.RAY_DTYPE
    for st, dt in ((_abi.Sight, generators.SIGHT_DTYPE), (_abi.SightRay, generators.SIGHT_RAY_DTYPE), (_abi.SightTarget, generators.SIGHT_TARGET_DTYPE)):
        assert [(n, getattr(st, n).offset) for n, _ in st._fields_] == [(n, dt.fields[n][1]) for n in dt.names]
    assert "hidden behind terrain" in header and "sight lines" in header


FANS = [(-5.0, 5.0), (-1.0, 1.0), (0.0, 1.0), (-0.3, 2.9), (1e-3, 1e-3 + 1e-9), (-90.0, 90.0), (0.1, 0.7),
        (0.25, np.nextafter(0.25, 1.0)), (-0.25, np.nextafter(-0.25, 1.0)), (1.0, np.nextafter(1.0, 2.0)),  # one ulp wide
        (-0.1, 0.1), (-2.0 / 3.0, 2.0 / 3.0), (-1e-12, 1e-12)]  # lo = -hi


@pytest.mark.parametrize("lo,hi", FANS)
def test_fan_angles_equal_the_numpy_expression(lib, lo, hi):
    got = generators.sight_fan_angles(lo, hi, lib)
    want = lo + np.arange(64, dtype=np.float64) * ((hi - lo) / 63.0)
    assert got.tobytes() == want.tobytes() == sm.fan_angles(lo, hi).tobytes(), (lo, hi, np.flatnonzero(got != want))
    assert got[0] == lo and (np.diff(got) >= 0).all()
    assert lib.atmrt_sight_fan_angles(lo, hi, None) == _abi.ERR_INVALID_ARGUMENT


def test_fan_angles_random_fans(lib):
    rng = np.random.default_rng(24)
    for _ in range(2000):
        lo = float(rng.uniform(-10, 10))
        hi = lo + float(10.0 ** rng.uniform(-14, 1.5))
        assert generators.sight_fan_angles(lo, hi, lib).tobytes() == sm.fan_angles(lo, hi).tobytes(), (lo, hi)


def test_pick_against_the_model(lib):
    patterns = {"all pass": np.zeros(64, bool), "all fail": np.ones(64, bool)}
    for k in (0, 31, 63):
        patterns[f"single {k}"] = np.arange(64) == k
    patterns["non-monotone"] = np.isin(np.arange(64), (0, 1, 2, 7, 9, 40, 12))  # ducting: rays cross, a failing ray above passing ones
    patterns["prefix"] = np.arange(64) < 17
    rng = np.random.default_rng(7)
    for i in range(200):
        patterns[f"random {i}"] = rng.uniform(size=64) < rng.uniform()
    want_fixed = {"all pass": 0, "all fail": 64, "single 0": 1, "single 31": 32, "single 63": 64, "non-monotone": 41, "prefix": 17}
    for name, fails in patterns.items():
        got = generators.sight_pick(fails, lib)
        assert got == sm.pick(fails), (name, got)
        if name in want_fixed:
            assert got == want_fixed[name], name
    # any non-zero byte fails
    raw = np.zeros(64, dtype=np.uint8)
    raw[5], raw[20] = 255, 2
    k = C.c_int32(-7)
    assert lib.atmrt_sight_pick(raw.ctypes.data, C.byref(k)) == 0 and k.value == 21
    assert lib.atmrt_sight_pick(None, C.byref(k)) == _abi.ERR_INVALID_ARGUMENT and lib.atmrt_sight_pick(raw.ctypes.data, None) == _abi.ERR_INVALID_ARGUMENT


def test_ctx_entry_points_refuse_a_null_context(lib):
    t = _abi.SightTarget(0.0, 1000.0, 0.0)
    out = _abi.Sight()
    ray = _abi.SightRay()
    ang = (C.c_double * 1)(0.0)
    assert lib.atmrt_sight_lines(None, C.byref(t), 1, -1.0, 1.0, 3, C.byref(out)) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_sight_fan_probe(None, C.byref(t), 1, ang, C.byref(ray)) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_last_sight_timings(None, (C.c_double * 3)()) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_last_sight_batches(None, C.byref(C.c_int32())) == _abi.ERR_INVALID_ARGUMENT


def test_csv_tables_and_the_pixel_inverse(tmp_path):
    src = tmp_path / "targets.csv"
    src.write_text("name,lat,lon,height\nPeak,46.9,8.5,30\n\nTower,46.7,8.6\nBare,46.6,8.4,\n")
    names, lat, lon, height = generators.read_sight_csv(str(src))
    assert names == ["Peak", "Tower", "Bare"] and lat.tolist() == [46.9, 46.7, 46.6] and height.tolist() == [30.0, 0.0, 0.0]
    (tmp_path / "bad.csv").write_text("A,46.9,8.5,tall\n")
    with pytest.raises(ValueError):
        generators.read_sight_csv(str(tmp_path / "bad.csv"))
    # the inverse of fast.rs:111-125 returns every pixel of a frame from that pixel's own direction and angle
    p = _abi.Params()
    p.width, p.height = 64, 48
    p.frame.direction, p.frame.fov, p.frame.tilt = 10.0, 60.0, -3.0
    for x in (0, 1, 31, 32, 63):
        for y in (0, 23, 24, 47):
            d = p.frame.direction + (x - p.width // 2) / p.width * p.frame.fov
            e = p.frame.tilt - (y - p.height // 2) / p.height * p.frame.fov / (p.width / p.height)
            assert generators.fast_pixel_of(p, d, e) == (x, y)
            assert generators.fast_pixel_of(p, d + 360.0, e) == (x, y)
    assert generators.fast_pixel_of(p, 10.0 + 31.0, -3.0) is None and generators.fast_pixel_of(p, 10.0, 30.0) is None
    assert generators.fast_pixel_of(p, 10.0, float("nan")) is None
    targets = np.zeros(2, dtype=generators.SIGHT_TARGET_DTYPE)
    targets["azimuth_deg"], targets["distance"] = (10.0, 200.0), (5000.0, 7000.0)
    sights = np.zeros(2, dtype=generators.SIGHT_DTYPE)
    sights["status"], sights["angle"], sights["hidden"] = (0, 2), (-3.0, np.nan), (0.001, np.nan)
    sights["block_distance"] = sights["block_lat"] = sights["block_lon"] = sights["block_elevation"] = np.nan
    buf = io.StringIO()
    generators.write_sight_csv(buf, ["a", "b"], targets, sights, p)
    rows = buf.getvalue().splitlines()
    assert rows[0].split(",") == list(generators.SIGHT_COLUMNS) and len(rows) == 3
    a, b = rows[1].split(","), rows[2].split(",")
    assert a[3] == "seen" and a[-2:] == ["32", "24"] and a[8:12] == [""] * 4
    assert b[3] == "above_fan" and b[4] == "" and b[-2:] == ["", ""]
