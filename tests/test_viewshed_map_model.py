"""tests/viewshed_map_model.py alone (the rule of include/atmrt.h, "viewshed map"), on planes tests/viewshed_model.py makes from the
oracle's primitives — scene S2, 60 km, step 100 m — and generators.viewshed_map_grid against the oracle's coords_at_dist.  No device."""
import ctypes as C

import numpy as np
import pytest

import sight_model as sm
import viewshed_map_model as mm
import viewshed_model as vm
from atm_raytracer_amd import _abi, _lib, generators, synth

FAN = (-6.0, 6.0)
N_AZ, REACH = 12, 60_000.0


@pytest.fixture(scope="module")
def s2(oracle_det):
    """The viewshed of scene S2 along 12 azimuths as far as 60 km, once."""
    cfg, tiles = synth.scene("S2", 64, 48, generator="Fast", max_distance=60_000.0)
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        v = vm.solve(setting, 0.0, 30.0, N_AZ, REACH, 0.0, FAN, 64)
    finally:
        setting.close()
    assert v["status"].shape == (N_AZ, 600) and cfg.params.simulation_step == 100.0
    return cfg, v


def bin_v(grid, v, into=None):
    return mm.bin_planes(grid, v["status"], v["hidden"], v["lat"], v["lon"], into)


def test_class_counts_add_up(s2):
    cfg, v = s2
    pos = cfg.params.position
    # a grid over the north-east quadrant only, a plane with NaN coordinates and statuses out of range mixed in
    grid = (pos.latitude, pos.longitude, 0.05, 0.05, 12, 18)
    status, lat = v["status"].copy(), v["lat"].copy()
    status[3, 10:20], lat[5, 100:130] = 7, np.nan
    n_samples, n_seen, min_hidden, st = mm.bin_planes(grid, status, v["hidden"], lat, v["lon"])
    print(f"viewshed map model classes: {st}")
    assert st["n_samples"] == N_AZ * 600 == st["n_binned"] + st["n_outside"] + st["n_skipped"]
    assert st["n_skipped"] == 40 and st["n_outside"] > 0 and st["n_binned"] > 0
    assert int(n_samples.sum()) == st["n_binned"] and int(n_seen.sum()) == st["n_seen"] and (n_seen <= n_samples).all()
    assert (np.isinf(min_hidden) | (min_hidden >= 0.0)).all() and np.isinf(min_hidden[n_samples == 0]).all() and np.isfinite(min_hidden).any()
    take = np.isin(v["status"], (vm.SEEN, vm.HIDDEN))
    assert (v["hidden"][take] >= 0.0).all() and not np.signbit(v["hidden"][take]).any()  # ray k* does not fail: the condition is idle here


def test_one_cell_over_everything_holds_every_sample(s2):
    _, v = s2
    n_samples, n_seen, min_hidden, st = bin_v((40.0, 0.0, 16.0, 16.0, 1, 1), v)
    assert n_samples.shape == (1, 1) and int(n_samples[0, 0]) == N_AZ * 600 == st["n_binned"] and st["n_outside"] == st["n_skipped"] == 0
    assert int(n_seen[0, 0]) == int(np.isin(v["status"], (vm.SEEN, vm.BELOW_FAN)).sum()) > 0
    take = np.isin(v["status"], (vm.SEEN, vm.HIDDEN))
    assert min_hidden[0, 0] == v["hidden"][take].min()
    # accumulating a map onto itself doubles the counts and keeps the minimum
    twice = bin_v((40.0, 0.0, 16.0, 16.0, 1, 1), v, into=(n_samples, n_seen, min_hidden))
    assert int(twice[0][0, 0]) == 2 * N_AZ * 600 and int(twice[1][0, 0]) == 2 * int(n_seen[0, 0]) and twice[2][0, 0] == min_hidden[0, 0]
    assert twice[3] == st  # stats are of the call


def test_half_cell_shift_follows_the_edge_rule(s2):
    """Cells of 2^-5 degrees on corners that are multiples of 2^-6: every quotient is exact, so the map over the cells of half the size
    decides both coarse maps — rows 2i, 2i + 1 make row i of the grid on the same corner, rows 2i + 1, 2i + 2 row i of the grid shifted
    north by half a cell — and columns likewise."""
    _, v = s2
    c = 2.0 ** -5
    fine = bin_v((45.0, 7.0, c / 2, c / 2, 192, 192), v)
    base = bin_v((45.0, 7.0, c, c, 96, 96), v)
    north = bin_v((45.0 + c / 2, 7.0, c, c, 96, 96), v)
    east = bin_v((45.0, 7.0 + c / 2, c, c, 96, 96), v)
    assert fine[3]["n_outside"] == 0 and base[3]["n_outside"] == 0
    for k in (0, 1):
        f = fine[k].astype(np.int64)
        assert np.array_equal(base[k], f[0::2][:, 0::2] + f[1::2][:, 0::2] + f[0::2][:, 1::2] + f[1::2][:, 1::2])
        rows = np.vstack([f[1:], np.zeros((1, 192), np.int64)])  # row r of `rows` is fine row r + 1
        assert np.array_equal(north[k], rows[0::2][:, 0::2] + rows[1::2][:, 0::2] + rows[0::2][:, 1::2] + rows[1::2][:, 1::2])
        cols = np.hstack([f[:, 1:], np.zeros((192, 1), np.int64)])
        assert np.array_equal(east[k], cols[0::2][:, 0::2] + cols[1::2][:, 0::2] + cols[0::2][:, 1::2] + cols[1::2][:, 1::2])
    assert north[3]["n_outside"] == int(fine[0][0].sum()) and east[3]["n_outside"] == int(fine[0][:, 0].sum())  # what lay in the first half row / column
    moved = int((base[0] != north[0]).sum())
    print(f"viewshed map model shift: {moved} of {base[0].size} cells differ between the grid and the one half a cell north")
    assert moved > 0
    # the edges themselves, on one sample's own coordinates: a cell half a degree high whose south edge is the sample's latitude holds
    # it, one whose north edge is that latitude does not; west and east likewise.  46.x - 0.5 and 8.x - 0.5 are exact.
    lib = _lib.load()
    lat, lon = float(v["lat"][2, 57]), float(v["lon"][2, 57])
    assert 32.5 < lat < 64.0 and 8.5 < lon < 16.0
    for grid, want in (((lat, lon, 0.5, 0.5, 1, 1), 0), ((lat - 0.5, lon, 0.5, 0.5, 1, 1), -1), ((lat, lon - 0.5, 0.5, 0.5, 1, 1), -1),
                       ((lat - 0.5, lon - 0.5, 0.5, 0.5, 2, 2), 3)):
        assert int(mm.cells(grid, np.float64(lat), np.float64(lon))) == want, grid
        assert generators.geo_grid_cell(_abi.GeoGrid(*grid), lat, lon, lib) == want, grid


def test_the_sea_inside_the_horizon_is_seen(oracle_det):
    """No tiles, the observer h = 100 m above a sea on the sphere, refraction on, height 0: inside the horizon distance every binned
    sample is seen — as far as the fan resolves it.  A sample at distance d is SEEN (not HIDDEN) when the highest ray under the
    surface there went under within that very step, that is when a ray sinks more against the surface in one step, step * (h / d -
    d / 2R'), than neighbouring rays lie apart, d * delta; that slope vanishes AT the horizon sqrt(2 R' h) (35.7 km for R' = R, more
    with refraction), so with any fan the last kilometres before it hold HIDDEN samples (at 4096 rays over 2 degrees: from 27 km on).
    Hence the shapes: 20 km, where a ray sinks 100 * (0.005 - 0.0016) = 0.34 m per step even without refraction (more with it), and
    4096 rays over 0.7 degrees, 20 km * 2.98e-6 rad = 0.06 m apart.  The fan's top ray (-0.3 degrees) lands beyond 20 km (the
    surface there lies at -0.38 degrees), so no sample is ABOVE_FAN; nearer than the lowest ray's landing no ray fails (BELOW_FAN)."""
    cfg, tiles = synth.scene("S1", 64, 48, straight_rays=False)
    assert not tiles and cfg.params.straight_rays == 0 and cfg.params.position.altitude == 100.0 and cfg.params.earth.radius == 6_371_000.0
    reach, fan, K = 20_000.0, (-1.0, -0.3), 4096
    horizon = np.sqrt(2.0 * 6_371_000.0 * 100.0)
    assert reach + cfg.params.simulation_step < horizon
    sink = cfg.params.simulation_step * (100.0 / (reach + 100.0) - (reach + 100.0) / (2.0 * 6_371_000.0))
    apart = (reach + 100.0) * np.radians((fan[1] - fan[0]) / (K - 1))
    assert sink > 4.0 * apart, (sink, apart)
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        v = vm.solve(setting, 0.0, 45.0, 8, reach, 0.0, fan, K)
    finally:
        setting.close()
    counts = np.bincount(v["status"].ravel(), minlength=4).tolist()
    pos = cfg.params.position
    grid = generators.viewshed_map_grid(pos.latitude, pos.longitude, float(v["d"][-1]), 30.0 / 3600.0)
    n_samples, n_seen, min_hidden, st = bin_v(grid, v)
    print(f"viewshed map model sea: seen/hidden/above/below {counts}, {st}, grid {grid.n_lat} x {grid.n_lon}")
    assert st["n_outside"] == 0 and st["n_binned"] == 8 * 200 and counts[vm.SEEN] > 0 and counts[vm.BELOW_FAN] > 0
    assert np.array_equal(n_seen, n_samples) and st["n_seen"] == st["n_binned"] and (n_samples > 0).sum() > 100


@pytest.mark.parametrize("lat,lon,reach,cell", [(46.5, 8.5, 60_000.0, 3.0 / 3600.0), (0.5, 0.5, 30_000.0, 30.0 / 3600.0), (-33.9, 151.2, 200_000.0, 0.01),
                                                (78.2, 15.6, 400_000.0, 0.05)])
def test_map_grid_holds_the_lattice_point_at_reach(oracle_det, lat, lon, reach, cell):
    """360 azimuths, the point at `reach` on the Spherical model of 6,371 km through the oracle's coords_at_dist: inside the grid, and
    not in its outermost ring of cells (the margin)."""
    earth = synth.scene("S1", 64, 48)[0].params.earth
    assert earth.radius == generators.VIEWSHED_MAP_RADIUS
    grid = generators.viewshed_map_grid(lat, lon, reach, cell)
    ll = np.array([oracle_det.coords_at_dist(earth, lat, lon, float(az), np.array([reach]))[0] for az in range(360)])
    lon_u = lon + (ll[:, 1] - lon + 180.0) % 360.0 - 180.0  # the grid's longitudes are plain numbers around the observer's
    cell_ix = mm.cells(grid, ll[:, 0], lon_u)
    i, j = cell_ix // grid.n_lon, cell_ix % grid.n_lon
    print(f"viewshed map grid {lat} {lon} reach {reach:g}: {grid.n_lat} x {grid.n_lon} cells, rows {i.min()}..{i.max()}, columns {j.min()}..{j.max()}")
    assert (cell_ix >= 0).all()
    assert i.min() >= 1 and i.max() <= grid.n_lat - 2 and j.min() >= 1 and j.max() <= grid.n_lon - 2
    assert int(mm.cells(grid, np.float64(lat), np.float64(lon))) >= 0
    # and no wider than it needs to be: the ring touches the extreme points within two cells
    assert i.min() <= 2 and i.max() >= grid.n_lat - 3 and j.min() <= 2 and j.max() >= grid.n_lon - 3
    assert C.sizeof(_abi.GeoGrid) == 40 and isinstance(grid, _abi.GeoGrid)
