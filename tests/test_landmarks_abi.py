"""The host half of the landmark search (include/atmrt.h): names and struct sizes, the rule atmrt_landmark_d2 against numpy bit for
bit, the refusals of the ctx-free entry points, the bucket index behind atmrt_landmark_index_probe (it may only ever ADD candidates
to what the brute-force rule admits, and it must be a filter), the CSV tables of the command line, and the numpy model's own
self-test (tests/landmarks_model.py).  The library loads without a GPU; nothing here touches a device."""
import ctypes as C
import io
import os
import re

import numpy as np
import pytest

import landmarks_model as lm
from atm_raytracer_amd import _abi, _lib, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_landmark_d2", "atmrt_locate_landmarks", "atmrt_locate_landmarks_planes_device", "atmrt_landmark_index_probe")
ARCSEC = 1.0 / 3600.0


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
    assert lib.atmrt_abi_sizeof(20) == C.sizeof(_abi.Landmark) == 24
    assert lib.atmrt_abi_sizeof(21) == C.sizeof(_abi.LandmarkHit) == generators.LANDMARK_HIT_DTYPE.itemsize == lm.HIT_DTYPE.itemsize == 40
    assert lib.atmrt_abi_sizeof(22) == C.sizeof(_abi.LandmarkStats) == 32
    assert lib.atmrt_abi_sizeof(23) == 0 and lib.atmrt_abi_version() == 5
    assert generators.LANDMARK_HIT_DTYPE == lm.HIT_DTYPE
    assert "hidden behind terrain" in header  # what "not found" does not tell apart


def test_landmark_d2_equals_the_numpy_rule(lib):
    rng = np.random.default_rng(20250118)
    n = 100_000
    l_lat, l_lon = rng.uniform(-80, 80, n), rng.uniform(-180, 180, n)
    scale = np.where(rng.integers(0, 4, n) == 0, rng.uniform(1e-6, 1.0, n), np.cos(np.radians(l_lat)))
    spread = 10.0 ** rng.uniform(-9, 0, n)  # from a fraction of an arcsecond to a degree away
    lat, lon = l_lat + rng.normal(0, 1, n) * spread, l_lon + rng.normal(0, 1, n) * spread
    same = rng.integers(0, 50, n) == 0
    lat[same], lon[same] = l_lat[same], l_lon[same]  # equal coordinates: d2 is +0.0
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e300, -1e300, 5e-324, 47.0])
    s_lat, s_lon = np.repeat(special, special.size), np.tile(special, special.size)
    l_lat = np.r_[l_lat, np.full(s_lat.size, 47.0), np.zeros(s_lat.size)]
    l_lon = np.r_[l_lon, np.full(s_lat.size, 8.0), np.full(s_lat.size, -0.0)]
    scale = np.r_[scale, np.full(s_lat.size, 0.6819983600624985), np.full(s_lat.size, 1.0)]
    lat, lon = np.r_[lat, s_lat, s_lat], np.r_[lon, s_lon, s_lon]
    want = lm.d2(l_lat, l_lon, scale, lat, lon)
    got = np.empty_like(want)
    out, mark = C.c_double(), _abi.Landmark()
    for i, (a, b, s, x, y) in enumerate(zip(l_lat.tolist(), l_lon.tolist(), scale.tolist(), lat.tolist(), lon.tolist())):
        mark.lat, mark.lon, mark.lon_scale = a, b, s
        assert lib.atmrt_landmark_d2(C.byref(mark), x, y, C.byref(out)) == 0
        got[i] = out.value
    gb, wb = got.view(np.uint64).copy(), want.view(np.uint64).copy()
    gb[np.isnan(got)] = wb[np.isnan(want)] = 0
    bad = np.flatnonzero(gb != wb)
    assert bad.size == 0, (bad.size, lat[bad[:5]], lon[bad[:5]], got[bad[:5]], want[bad[:5]])
    assert np.isnan(want).sum() > 10 and np.isposinf(want).sum() > 10 and (want == 0).sum() > 1000 and not np.signbit(want[want == 0]).any()
    assert generators.landmark_d2(generators.landmarks([47.0], [8.0], 1.0)[0], 47.0 + 3 / 1024, 8.0 + 4 / 1024, lib) == 25 / 1024 ** 2


def test_landmarks_mirror():
    arr = generators.landmarks([47.0, -33.5], [8.0, 151.25])
    assert len(arr) == 2 and arr[1].lat == -33.5 and arr[1].lon == 151.25
    assert arr[0].lon_scale == np.cos(np.radians(47.0)) == generators.landmark_scale(47.0)
    assert generators.landmarks([1.0, 2.0], [3.0, 4.0], 0.5)[1].lon_scale == 0.5
    with pytest.raises(ValueError):
        generators.landmarks([1.0, 2.0], [3.0])


def probe(lib, marks, radius, bounds, lat, lon, capacity=None, n=None):
    lat, lon = np.ascontiguousarray(lat, dtype=np.float64), np.ascontiguousarray(lon, dtype=np.float64)
    offsets = np.full(lat.size + 1, 77, dtype=np.uint64)
    items = np.full(64 if capacity is None else max(capacity, 1), 77, dtype=np.uint32)
    need = C.c_size_t(77)
    rc = lib.atmrt_landmark_index_probe(marks, len(marks) if n is None else n, radius, (C.c_double * 4)(*bounds), lat.ctypes.data, lon.ctypes.data,
                                        lat.size, offsets.ctypes.data, items.ctypes.data, items.size if capacity is None else capacity, C.byref(need))
    return rc, need.value, offsets, items


def test_ctx_free_entry_points_refuse_bad_arguments(lib):
    out = C.c_double(7.0)
    ok = generators.landmarks([47.0, 47.5], [8.0, 8.5])
    assert lib.atmrt_landmark_d2(None, 47.0, 8.0, C.byref(out)) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_landmark_d2(C.byref(ok[0]), 47.0, 8.0, None) == _abi.ERR_INVALID_ARGUMENT and out.value == 7.0
    bounds, lat, lon = (46.9, 47.6, 7.9, 8.6), np.array([47.0, 47.5, 47.25]), np.array([8.0, 8.5, 8.25])
    rc, need, offsets, items = probe(lib, ok, 3 * ARCSEC, bounds, lat, lon)
    assert rc == 0 and need == 2 and offsets.tolist() == [0, 1, 2, 2] and items[:2].tolist() == [0, 1]
    # too small a capacity: the need is reported, nothing else written
    rc, need, offsets, items = probe(lib, ok, 3 * ARCSEC, bounds, lat, lon, capacity=1)
    assert rc == _abi.ERR_INVALID_ARGUMENT and need == 2 and (offsets == 77).all() and (items == 77).all()
    assert probe(lib, ok, 3 * ARCSEC, bounds, lat, lon, n=0)[0] == _abi.ERR_INVALID_ARGUMENT
    assert probe(lib, ok, 3 * ARCSEC, bounds, lat, lon, n=(1 << 20) + 1)[0] == _abi.ERR_INVALID_ARGUMENT
    for radius in (0.0, -1.0, float("nan"), float("inf"), 1.0000001):
        assert probe(lib, ok, radius, bounds, lat, lon)[0] == _abi.ERR_INVALID_ARGUMENT, radius
    assert probe(lib, ok, 1.0, bounds, lat, lon, capacity=16)[0] == 0
    for field, value in (("lat", float("nan")), ("lat", float("inf")), ("lon", float("-inf")), ("lon", float("nan")), ("lon_scale", 0.0),
                         ("lon_scale", 0.9e-6), ("lon_scale", 1.0000001), ("lon_scale", float("nan")), ("lon_scale", -0.5)):
        bad = generators.landmarks([47.0, 47.5], [8.0, 8.5])
        setattr(bad[1], field, value)
        assert probe(lib, bad, 3 * ARCSEC, bounds, lat, lon)[0] == _abi.ERR_INVALID_ARGUMENT, (field, value)
    need = C.c_size_t()
    b, o, it = (C.c_double * 4)(*bounds), np.zeros(4, dtype=np.uint64), np.zeros(8, dtype=np.uint32)
    args = lambda **kw: [kw.get("marks", ok), 2, 3 * ARCSEC, kw.get("b", b), kw.get("lat", lat.ctypes.data), kw.get("lon", lon.ctypes.data), 3,
                         kw.get("o", o.ctypes.data), kw.get("it", it.ctypes.data), 8, kw.get("need", C.byref(need))]
    assert lib.atmrt_landmark_index_probe(*args()) == 0
    for null in ("marks", "b", "lat", "lon", "o", "it", "need"):
        assert lib.atmrt_landmark_index_probe(*args(**{null: None})) == _abi.ERR_INVALID_ARGUMENT, null


def admitted_pairs(marks, radius, lat, lon):
    """The brute-force rule over every (point, landmark) pair -> a sorted array of point * n + landmark.  To spare a 10^9-element
    table, a landmark is only paired with the points whose latitude lies within 2 radius of its own: beyond that dlat * dlat alone is
    nearly 4 r2, so the rule cannot admit the pair whatever the rounding."""
    l_lat, l_lon, l_scale = lm.landmark_arrays(marks)
    order = np.argsort(lat, kind="stable")
    s_lat = lat[order]
    lo, hi = np.searchsorted(s_lat, l_lat - 2 * radius, "left"), np.searchsorted(s_lat, l_lat + 2 * radius, "right")
    which = np.repeat(np.arange(l_lat.size), hi - lo)
    pt = order[np.arange((hi - lo).sum()) - np.repeat(np.cumsum(hi - lo) - (hi - lo), hi - lo) + np.repeat(lo, hi - lo)]
    ok = lm.within(l_lat[which], l_lon[which], l_scale[which], lat[pt], lon[pt], radius)
    return np.sort(pt[ok].astype(np.int64) * l_lat.size + which[ok])


def candidate_pairs(lib, marks, radius, bounds, lat, lon):
    offsets, items = generators.landmark_index_probe(marks, radius, bounds, lat, lon, lib)
    assert offsets[0] == 0 and offsets[-1] == items.size and (np.diff(offsets.astype(np.int64)) >= 0).all()
    assert items.size == 0 or items.max() < len(marks)
    pt = np.repeat(np.arange(lat.size, dtype=np.int64), np.diff(offsets.astype(np.int64)))
    return pt * len(marks) + items, offsets


BOX = (47.0, 48.0, 8.0, 9.5)  # 1 x 1.5 degrees at 47 N


@pytest.fixture(scope="module")
def uniform():
    rng = np.random.default_rng(4711)
    marks = generators.landmarks(rng.uniform(BOX[0], BOX[1], 10_000), rng.uniform(BOX[2], BOX[3], 10_000))
    return marks, rng.uniform(BOX[0], BOX[1], 100_000), rng.uniform(BOX[2], BOX[3], 100_000)


def test_index_never_loses_a_pair_uniform_population(lib, uniform):
    marks, lat, lon = uniform
    radius = 3 * ARCSEC
    l_lat, l_lon, l_scale = lm.landmark_arrays(marks)
    rng = np.random.default_rng(12)
    # points on the natural edges of an index with cells of 2 radius laid from the corner of the bounds, one ulp to either side of
    # them, on the edges of the landmarks' own boxes, and on the bounds themselves
    k = rng.integers(0, 600, 400)
    e_lat = BOX[0] + k * (2 * radius)
    e_lon = BOX[2] + rng.integers(0, 600, 400) * (2 * radius / l_scale.max())
    pick = rng.integers(0, l_lat.size, 400)
    extra_lat = np.r_[e_lat, np.nextafter(e_lat, -np.inf), np.nextafter(e_lat, np.inf), l_lat[pick], l_lat[pick] + radius, l_lat[pick] - radius,
                      l_lat[pick], l_lat[pick], [BOX[0], BOX[0], BOX[1], BOX[1]]]
    extra_lon = np.r_[l_lon[pick], l_lon[pick], l_lon[pick], e_lon, l_lon[pick], l_lon[pick], l_lon[pick] + radius / l_scale[pick],
                      l_lon[pick] - radius / l_scale[pick], [BOX[2], BOX[3], BOX[2], BOX[3]]]
    inside = (extra_lat >= BOX[0]) & (extra_lat <= BOX[1]) & (extra_lon >= BOX[2]) & (extra_lon <= BOX[3])  # a frame's points lie within its bounds
    assert inside.sum() > 3000
    lat, lon = np.r_[lat, extra_lat[inside]], np.r_[lon, extra_lon[inside]]
    want = admitted_pairs(marks, radius, lat, lon)
    got, _ = candidate_pairs(lib, marks, radius, BOX, lat, lon)
    missing = np.setdiff1d(want, got)
    print(f"landmark index, uniform + edges: {lat.size} points, {len(marks)} landmarks, {want.size} admitted pairs, {got.size} candidates, {missing.size} missing")
    assert want.size > 1000 and missing.size == 0, (missing[:5] // len(marks), missing[:5] % len(marks))


def test_index_never_loses_a_pair_on_the_radius(lib):
    """Exactly representable offsets: dlat = 3 * 2^-10, dlon * scale = 4 * 2^-10, radius = 5 * 2^-10, so d2 == r2 to the bit and the
    point is within; its nextafter neighbours away from the landmark are not."""
    radius, u = 5.0 / 1024, 1.0 / 1024
    gi, gj = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    l_lat, l_lon = 47.0 + gi.ravel() / 16.0, 8.0 + gj.ravel() / 16.0
    scale = np.where((gi + gj).ravel() % 2 == 0, 1.0, 0.5)
    marks = generators.landmarks(l_lat, l_lon, scale)
    sgn = np.array([(1, 1), (1, -1), (-1, 1), (-1, -1)])
    on_lat = (l_lat[:, None] + sgn[None, :, 0] * 3 * u).ravel()
    on_lon = (l_lon[:, None] + sgn[None, :, 1] * 4 * u / scale[:, None]).ravel()
    out_lat = np.nextafter(on_lat, on_lat + np.tile(sgn[:, 0], l_lat.size))
    out_lon = np.nextafter(on_lon, on_lon + np.tile(sgn[:, 1], l_lat.size))
    own = np.repeat(np.arange(l_lat.size), 4)
    assert (lm.d2(l_lat[own], l_lon[own], scale[own], on_lat, on_lon) == radius * radius).all()
    assert lm.within(l_lat[own], l_lon[own], scale[own], on_lat, on_lon, radius).all()
    assert not lm.within(l_lat[own], l_lon[own], scale[own], out_lat, on_lon, radius).any()
    assert not lm.within(l_lat[own], l_lon[own], scale[own], on_lat, out_lon, radius).any()
    lat, lon = np.r_[on_lat, out_lat, on_lat], np.r_[on_lon, on_lon, out_lon]
    assert lat.size >= 1000
    bounds = (lat.min(), lat.max(), lon.min(), lon.max())
    want = admitted_pairs(marks, radius, lat, lon)
    got, _ = candidate_pairs(lib, marks, radius, bounds, lat, lon)
    missing = np.setdiff1d(want, got)
    print(f"landmark index, on the radius: {lat.size} points, {want.size} admitted pairs, {got.size} candidates, {missing.size} missing")
    assert np.isin(np.arange(on_lat.size) * len(marks) + own, want).all()
    assert missing.size == 0, (missing[:5] // len(marks), missing[:5] % len(marks))
    # bounds that cut through the landmarks' boxes: the points inside them keep their pairs
    inside = (lat >= 47.3) & (lat <= 47.6) & (lon >= 8.2) & (lon <= 8.7)
    want = admitted_pairs(marks, radius, lat[inside], lon[inside])
    got, _ = candidate_pairs(lib, marks, radius, (47.3, 47.6, 8.2, 8.7), lat[inside], lon[inside])
    assert want.size > 50 and np.setdiff1d(want, got).size == 0


def test_index_is_a_filter(lib, uniform):
    """About 9,800 landmarks per square degree (in lat x scaled lon) against a catchment of (4 r)^2 is 0.1 candidates per point with
    cells of 2 r; 1.0 leaves room for cells up to about 10 r and fails an index that degenerates towards brute force's 10,000."""
    marks, lat, lon = uniform
    _, offsets = candidate_pairs(lib, marks, 3 * ARCSEC, BOX, lat, lon)
    mean = float(offsets[-1]) / lat.size
    print(f"landmark index: {mean:.4f} candidates per point on the uniform population ({int(offsets[-1])} for {lat.size} points)")
    assert mean <= 1.0


def test_landmarks_outside_the_bounds_have_no_candidates(lib):
    rng = np.random.default_rng(3)
    far_lat = np.r_[rng.uniform(50.0, 51.0, 50), rng.uniform(47.0, 48.0, 50), 47.0 - 4 * ARCSEC, 48.0 + 4 * ARCSEC, 47.5, 47.5]
    far_lon = np.r_[rng.uniform(8.0, 9.5, 50), rng.uniform(12.0, 13.0, 50), 8.5, 8.5, 8.0 - 5 * ARCSEC, 9.5 + 5 * ARCSEC]
    near_lat, near_lon = rng.uniform(47.0, 48.0, 100), rng.uniform(8.0, 9.5, 100)
    lat, lon = np.r_[far_lat, near_lat, rng.uniform(47.0, 48.0, 2000)], np.r_[far_lon, near_lon, rng.uniform(8.0, 9.5, 2000)]
    # only landmarks whose boxes miss the bounds: no candidate at all, not even for the points that sit on them
    offsets, items = generators.landmark_index_probe(generators.landmarks(far_lat, far_lon), 3 * ARCSEC, BOX, lat, lon, lib)
    assert items.size == 0 and not offsets.any()
    # mixed with landmarks inside: the outside ones never show up, the inside ones find the points that sit on them
    marks = generators.landmarks(np.r_[far_lat, near_lat], np.r_[far_lon, near_lon])
    offsets, items = generators.landmark_index_probe(marks, 3 * ARCSEC, BOX, lat, lon, lib)
    assert items.size >= 100 and items.min() >= far_lat.size
    for i in range(100):
        assert far_lat.size + i in items[int(offsets[far_lat.size + i]):int(offsets[far_lat.size + i + 1])]
    # bounds without a point (a frame of sky)
    offsets, items = generators.landmark_index_probe(marks, 3 * ARCSEC, (float("nan"),) * 4, lat, lon, lib)
    assert items.size == 0


def test_csv_tables(tmp_path):
    p = tmp_path / "peaks.csv"
    p.write_text('name,lat,lon\nDom,46.0939,7.8586\n"Piz Bernina, east",46.3822,9.9081\n\nTödi, 46.8111 , 8.9147\n')
    names, lat, lon = generators.read_landmarks_csv(str(p))
    assert names == ["Dom", "Piz Bernina, east", "Tödi"] and lat.tolist() == [46.0939, 46.3822, 46.8111] and lon.tolist() == [7.8586, 9.9081, 8.9147]
    p.write_text("Dom,46.0939,7.8586\n")  # no header line
    assert generators.read_landmarks_csv(str(p))[0] == ["Dom"]
    p.write_text("name,lat,lon\nDom,46.0939,east\n")
    with pytest.raises(ValueError):
        generators.read_landmarks_csv(str(p))
    p.write_text("Dom,46.0939\n")
    with pytest.raises(ValueError):
        generators.read_landmarks_csv(str(p))
    hits = np.zeros(3, dtype=generators.LANDMARK_HIT_DTYPE)
    hits[0] = (5, 17, 9, 1, (3 * ARCSEC) ** 2, 41234.5, 4545.0)
    hits[1] = lm.NONE
    hits[2] = (1, 0, 0, 0, 0.0, 0.1, -3.25)
    f = io.StringIO()
    generators.write_landmarks_csv(f, names, lat, lon, hits)
    rows = f.getvalue().split("\n")
    assert rows[0] == "name,lat,lon,found,x,y,point,offset_arcsec,distance_m,elevation_m,n_within" == ",".join(generators.LANDMARK_COLUMNS)
    assert rows[1] == f"Dom,46.0939,7.8586,1,17,9,1,{float(np.sqrt((3 * ARCSEC) ** 2) * 3600.0)!r},41234.5,4545.0,5"
    assert rows[2] == '"Piz Bernina, east",46.3822,9.9081,0,,,,,,,0'
    assert rows[3] == "Tödi,46.8111,8.9147,1,0,0,0,0.0,0.1,-3.25,1" and rows[4] == "" and len(rows) == 5


def test_model_on_hand_made_arrays():
    """Ties across pixels and inside a pixel, skipped points, duplicate landmarks, no point within."""
    u = 1.0 / 1024
    # 2 x 3 pixels; pixel 1 holds three points (lists), pixel 4 two
    res = {"hit_count": np.array([[1, 3, 0], [1, 2, 1]], dtype=np.uint32), "hit_offset": np.array([[0, 1, 4], [4, 5, 7]], dtype=np.uint64),
           #                 p0        p1.0      p1.1      p1.2      p3        p4.0      p4.1    p5
           "lat": np.array([47 + 3 * u, 47 - 3 * u, 47 + 3 * u, 47.0, 47 - 3 * u, np.nan, 47.0, 47.0]),
           "lon": np.array([8 + 4 * u, 8 + 4 * u, 8 - 4 * u, 8.0, 8 - 4 * u, 8.0, 8.0, 8.0]),
           "distance": np.array([10.0, 11.0, 12.0, -1.0, 13.0, 14.0, np.nan, -0.0]),
           "elevation": np.array([100.0, 101.0, 102.0, 103.0, 104.0, 105.0, 106.0, 107.0])}
    marks = [(47.0, 8.0, 1.0), (47.0, 8.0, 1.0), (47.0, 8.0 + 8 * u, 1.0), (40.0, 8.0, 1.0), (47.0, 8.0, 0.5)]
    first, st = lm.locate(res, marks, 5 * u, "first")
    # FIRST: p0, p1.0, p3, p4.0 (NaN lat: skipped), p5 (distance -0.0: not skipped, d2 0)
    assert st == {"n_points": 5, "n_skipped": 1, "n_within": 4 + 4 + 2 + 0 + 4}
    assert first[0].tolist() == (4, 2, 1, 0, 0.0, -0.0, 107.0) and first[1].tolist() == first[0].tolist()
    assert first[2].tolist() == (2, 0, 0, 0, 25 * u * u, 10.0, 100.0)  # p0 and p1.0 tie at d2 == r2: the smaller pixel
    assert first[3]["n_within"] == 0 and first[3]["x"] == first[3]["y"] == 0xFFFFFFFF and np.isposinf(first[3]["d2"]) and np.isnan(first[3]["distance"])
    assert first[4]["n_within"] == 4 and first[4]["d2"] == 0.0
    every, st = lm.locate(res, marks, 5 * u, "all")
    # ALL: p1.2 (negative distance), p4.0 and p4.1 are skipped; p1.1 joins
    assert st["n_points"] == 8 and st["n_skipped"] == 3 and every[0]["n_within"] == 5
    tie, _ = lm.locate(res, [(47.0 + 6 * u, 8.0, 1.0)], 5 * u, "all")  # p0 and p1.1 at d2 = 25 u^2, the others farther: p0 wins
    assert tie[0].tolist() == (2, 0, 0, 0, 25 * u * u, 10.0, 100.0)
    tie, _ = lm.locate(res, [(47.0, 8.0 + 4 * u, 1.0)], 3 * u, "all")  # p0 and p1.0 at d2 = 9 u^2
    assert tie[0].tolist() == (2, 0, 0, 0, 9 * u * u, 10.0, 100.0)
    tie, _ = lm.locate(res, [(47.0, 8.0 - 4 * u, 1.0)], 3 * u, "all")  # p1.1 and p3 at d2 = 9 u^2: pixel 1, its point 1
    assert tie[0].tolist() == (2, 1, 0, 1, 9 * u * u, 12.0, 102.0)
    inside = dict(res, lat=np.array([47.0, 47.0, 47.0, 47.0, 47.0, 47.0, 47.0, 47.0]), distance=np.arange(8.0))
    tie, _ = lm.locate(inside, [(47.0, 8.0, 1.0)], 1 * u, "all")  # p1.2, p4.0, p4.1, p5 at d2 == 0: pixel 1, its point 2
    assert tie[0].tolist() == (4, 1, 0, 2, 0.0, 3.0, 103.0)
    lm.assert_records(every, every.copy())
    with pytest.raises(AssertionError):
        lm.assert_records(every, first)
