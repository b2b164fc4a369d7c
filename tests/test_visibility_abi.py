"""The host half of the visibility map (include/atmrt.h): the new names in the header, the loader and the library, the struct
sizes, and the binning rule atmrt_geo_grid_cell against numpy's np.floor((lat - lat0) / cell) (tests/visibility_model.py), index
for index.  The library loads without a GPU; nothing here touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import visibility_model as vm
from atm_raytracer_amd import _abi, _lib, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_geo_grid_cell", "atmrt_frame_bounds", "atmrt_visibility_map_device", "atmrt_visibility_map",
         "atmrt_visibility_map_planes_device")


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
    assert lib.atmrt_abi_sizeof(18) == C.sizeof(_abi.GeoGrid) == 40
    assert lib.atmrt_abi_sizeof(19) == C.sizeof(_abi.VisibilityStats) == 40
    assert lib.atmrt_abi_sizeof(17) == 0 and lib.atmrt_abi_version() == 5
    assert (_abi.VIS_FIRST, _abi.VIS_ALL) == (0, 1)
    assert "antimeridian" in header


def edge_points(g, rng):
    """Points exactly on every edge of the grid (the top and right ones are outside), on inner cell boundaries, one ulp to either
    side of them, and the special values."""
    lat_edges = g.lat0 + np.arange(g.n_lat + 1) * g.cell_lat
    lon_edges = g.lon0 + np.arange(g.n_lon + 1) * g.cell_lon
    lat_in = g.lat0 + rng.uniform(0, g.n_lat, 64) * g.cell_lat
    lon_in = g.lon0 + rng.uniform(0, g.n_lon, 64) * g.cell_lon
    lats, lons = [], []
    for e in (lat_edges, np.nextafter(lat_edges, -np.inf), np.nextafter(lat_edges, np.inf)):
        sel = e[np.unique(np.r_[0, 1, len(e) // 2, len(e) - 2, len(e) - 1, rng.integers(0, len(e), 24)])]
        lats.append(np.repeat(sel, 8)), lons.append(rng.choice(np.r_[lon_in, lon_edges[[0, -1]]], sel.size * 8))
    for e in (lon_edges, np.nextafter(lon_edges, -np.inf), np.nextafter(lon_edges, np.inf)):
        sel = e[np.unique(np.r_[0, 1, len(e) // 2, len(e) - 2, len(e) - 1, rng.integers(0, len(e), 24)])]
        lons.append(np.repeat(sel, 8)), lats.append(rng.choice(np.r_[lat_in, lat_edges[[0, -1]]], sel.size * 8))
    special = np.array([np.nan, np.inf, -np.inf, 1e300, -1e300, 0.0, -0.0])
    lats.append(np.repeat(special, special.size)), lons.append(np.tile(special, special.size))
    lats.append(special), lons.append(np.full(special.size, lon_in[0]))
    lats.append(np.full(special.size, lat_in[0])), lons.append(special)
    return np.concatenate(lats), np.concatenate(lons)


GRIDS = {
    "arcsec3": _abi.GeoGrid(46.0, 8.0, 1.0 / 1200.0, 1.0 / 1200.0, 1200, 1200),  # a cell size that is no power of two
    "pow2": _abi.GeoGrid(-0.5, -0.25, 1.0 / 64.0, 1.0 / 128.0, 64, 96),          # straddles 0: -0.0 and tiny negatives
    "one": _abi.GeoGrid(45.0, 7.0, 3.0, 4.0, 1, 1),
    "uneven": _abi.GeoGrid(-33.3, 151.1, 0.1 / 3.0, 0.07, 17, 4001),
    "large": _abi.GeoGrid(-90.0, -180.0, 180.0 / 32768.0, 360.0 / 65536.0, 32768, 65536),  # 2^31 cells: the largest index
}


@pytest.mark.parametrize("name", sorted(GRIDS))
def test_geo_grid_cell_equals_the_numpy_rule(lib, name):
    g = GRIDS[name]
    rng = np.random.default_rng(20250117 + sorted(GRIDS).index(name))
    e_lat, e_lon = edge_points(g, rng)
    n = 100_000 // len(GRIDS) - e_lat.size
    assert n > 10_000
    # uniform over the grid and a margin of a fifth of its extent on every side
    lat = g.lat0 + rng.uniform(-0.2, 1.2, n) * g.n_lat * g.cell_lat
    lon = g.lon0 + rng.uniform(-0.2, 1.2, n) * g.n_lon * g.cell_lon
    lat, lon = np.r_[e_lat, lat], np.r_[e_lon, lon]
    got = generators.geo_grid_cell(g, lat, lon, lib)
    want = vm.cells(g, lat, lon)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad.size, lat[bad[:5]], lon[bad[:5]], got[bad[:5]], want[bad[:5]])
    inside = want >= 0
    assert 0.3 < inside.mean() < 0.7 and want.max() < g.n_lat * g.n_lon
    # the edges themselves: bottom and left are inside, top and right outside
    mid_lon, mid_lat = g.lon0 + 0.5 * g.cell_lon, g.lat0 + 0.5 * g.cell_lat
    top, right = g.lat0 + g.n_lat * g.cell_lat, g.lon0 + g.n_lon * g.cell_lon
    assert generators.geo_grid_cell(g, g.lat0, g.lon0, lib) == 0
    assert vm.cells(g, top, mid_lon) == -1 and generators.geo_grid_cell(g, top, mid_lon, lib) == -1
    assert vm.cells(g, mid_lat, right) == -1 and generators.geo_grid_cell(g, mid_lat, right, lib) == -1
    for v in (np.nan, np.inf, -np.inf, 1e300):
        assert generators.geo_grid_cell(g, v, mid_lon, lib) == -1 and generators.geo_grid_cell(g, mid_lat, v, lib) == -1


def test_total_of_the_sweep_is_1e5_points():
    assert 100_000 // len(GRIDS) * len(GRIDS) == 100_000


def test_geo_grid_cell_refuses_bad_grids(lib):
    cell = C.c_int64(7)
    ok = _abi.GeoGrid(46.0, 8.0, 0.5, 0.5, 2, 2)
    assert lib.atmrt_geo_grid_cell(C.byref(ok), 46.6, 8.6, C.byref(cell)) == 0 and cell.value == 3
    assert lib.atmrt_geo_grid_cell(None, 46.6, 8.6, C.byref(cell)) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_geo_grid_cell(C.byref(ok), 46.6, 8.6, None) == _abi.ERR_INVALID_ARGUMENT
    for bad in bad_grids():
        cell.value = 7
        assert lib.atmrt_geo_grid_cell(C.byref(bad), 46.6, 8.6, C.byref(cell)) == _abi.ERR_INVALID_ARGUMENT
        assert cell.value == -1
        with pytest.raises(_lib.AtmrtError):
            generators.geo_grid_cell(bad, 46.6, 8.6, lib)
    full = _abi.GeoGrid(0.0, 0.0, 1.0, 1.0, 1 << 15, 1 << 16)  # exactly 2^31 cells is allowed
    assert lib.atmrt_geo_grid_cell(C.byref(full), 32767.5, 65535.5, C.byref(cell)) == 0 and cell.value == (1 << 31) - 1


def bad_grids():
    """Every grid section 4 of the feature's description refuses."""
    out = []
    for k in ("cell_lat", "cell_lon"):
        for v in (0.0, -0.5, float("nan"), float("inf")):
            g = _abi.GeoGrid(46.0, 8.0, 0.5, 0.5, 2, 2)
            setattr(g, k, v)
            out.append(g)
    for k in ("lat0", "lon0"):
        for v in (float("nan"), float("inf"), float("-inf")):
            g = _abi.GeoGrid(46.0, 8.0, 0.5, 0.5, 2, 2)
            setattr(g, k, v)
            out.append(g)
    out.append(_abi.GeoGrid(46.0, 8.0, 0.5, 0.5, 0, 2))
    out.append(_abi.GeoGrid(46.0, 8.0, 0.5, 0.5, 2, 0))
    out.append(_abi.GeoGrid(46.0, 8.0, 0.5, 0.5, (1 << 15) + 1, 1 << 16))  # 2^31 + 2^16 cells
    out.append(_abi.GeoGrid(46.0, 8.0, 0.5, 0.5, 0xFFFFFFFF, 0xFFFFFFFF))
    return out


def test_snap_grid_covers_its_bounds():
    rng = np.random.default_rng(5)
    for _ in range(200):
        cell = float(rng.choice([1.0 / 1200.0, 30.0 / 3600.0, 1.0 / 3600.0, 0.25]))
        lat_min, lon_min = float(rng.uniform(-60, 60)), float(rng.uniform(-170, 170))
        if rng.integers(0, 3) == 0:  # bounds that sit exactly on multiples of the cell
            lat_min, lon_min = float(np.floor(lat_min / cell)) * cell, float(np.floor(lon_min / cell)) * cell
        b = (lat_min, lat_min + float(rng.uniform(0, 1.5)), lon_min, lon_min + float(rng.uniform(0, 1.5)))
        g = generators.snap_grid(b, cell)
        corners = vm.cells(g, np.array([b[0], b[0], b[1], b[1]]), np.array([b[2], b[3], b[2], b[3]]))
        assert (corners >= 0).all(), (b, cell)
        assert abs(g.lat0 / cell - round(g.lat0 / cell)) < 1e-6 and g.lat0 <= b[0] < g.lat0 + 2 * cell
    assert generators.snap_grid((float("nan"),) * 4, 0.1) is None
