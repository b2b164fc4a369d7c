"""The terrain ceiling table (csrc/atmrt_ceiling.h) on the host, before any kernel trusts it: tests/csrc/ceiling_host.cpp, a stand-alone
program, fills the table for a small mosaic with the functions the device kernels run and attacks every cell with seeded directions
(inside each bin, at its edges, one rounding step to either side of them) at every step: the product's own lookup at the ray's
geodesic point must lie the table's 1 m margin below the cell and the suffix of the ray's bin, every cell must have been attacked,
and the suffix must be the running maximum.  The same sample points then go through the oracle's lookup, so that the product does
not only check itself.  A table of global tops cannot pass: on a mosaic of zeros with one 3000 m post every cell whose box (end
points from the oracle's geodesic, inflated by the arc's sagitta and two posts) does not hold that post must be 1 m.  A second build
runs one case under the address and undefined-behaviour sanitizers."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import cbuild
from oracle_binding import Oracle, _abi

FLAGS = ["g++", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]
RADIUS = 6_371_000.0
W, H, FOV = 64, 32, 12.0
HEADER = os.path.join(cbuild.HERE, "..", "atm-raytracer_amd", "csrc", "atmrt_ceiling.h")


def _exe(name, flags):
    out = os.path.join(cbuild.OUT, name)
    if os.path.exists(out) and os.path.getmtime(HEADER) > os.path.getmtime(out):
        os.remove(out)  # cbuild knows the core headers only
    return cbuild._build("ceiling_host.cpp", name, FLAGS + flags)


def _rough(seed, n_lat, n_lon):
    """posts without any smoothness: neighbours differ by up to 3000 m, the hardest ground for a bound taken from a box"""
    return np.random.default_rng(seed).integers(-50, 3000, size=(n_lat, n_lon)).astype(np.int16)


def _run(exe, tmp_path, tiles, lat, lon, direction, step, max_distance, tilt=0.0, per_cell=3, seed=1, fov=FOV, radius=RADIUS, width=W, height=H):
    case, out = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("<12d", lat, lon, direction, fov, tilt, step, max_distance, radius, width, height, per_cell, seed))
        f.write(struct.pack("<i", len(tiles)))
        for (la, lo), posts in tiles.items():
            f.write(struct.pack("<4i", la, lo, posts.shape[0], posts.shape[1]))
            f.write(np.ascontiguousarray(posts, dtype="<i2").tobytes())
    p = subprocess.run([exe, case, out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    words = p.stdout.split()
    stat = {words[k]: int(words[k + 1]) for k in range(0, len(words), 2)}
    with open(out, "rb") as f:
        rows, bins = struct.unpack("<2i", f.read(8))
        dir0, rel_lo, w = struct.unpack("<3d", f.read(24))
        xs = np.frombuffer(f.read(8 * rows), dtype="<f8")
        cell = np.frombuffer(f.read(4 * rows * (bins + 1)), dtype="<f4").reshape(rows, bins + 1)
        suffix = np.frombuffer(f.read(4 * rows * (bins + 1)), dtype="<f4").reshape(rows, bins + 1)
        (n,) = struct.unpack("<q", f.read(8))
        samples = np.frombuffer(f.read(32 * n), dtype="<f8").reshape(n, 4)
        where = np.frombuffer(f.read(12 * n), dtype="<i4").reshape(n, 3)  # step, bin, number within the cell
        assert len(where) == n and not f.read(1)
    assert stat["rows"] == rows and stat["bins"] == bins and stat["samples"] == n and stat["bad"] == 0 and stat["uncovered"] == 0
    assert n >= rows * bins * (per_cell + 2)
    return dict(stat=stat, xs=xs, cell=cell, suffix=suffix, samples=samples, where=where, layout=(dir0, rel_lo, w))


def _oracle_agrees(oracle, tiles, samples):
    t = oracle.terrain_new(tiles)
    try:
        for lat, lon, cell, suffix in samples:
            e = oracle.get_elev(t, lat, lon)
            e = 0.0 if e is None else e
            assert e <= cell - 1.0 + 1e-6 and e <= suffix - 1.0 + 1e-6, (lat, lon, e, cell, suffix)
    finally:
        oracle.terrain_free(t)


@pytest.fixture(scope="module")
def exe():
    return _exe("ceiling_host", ["-O2"])


@pytest.fixture(scope="module")
def oracle():
    return Oracle("det")


def _mosaic(cells, n=301, seed=7, skip=()):
    return {c: _rough(seed + 31 * k, n, n) for k, c in enumerate(cells) if c not in skip}


NINE = [(la, lo) for la in (45, 46, 47) for lo in (7, 8, 9)]
CASES = {
    # name: (tiles, observer lat, lon, yaw, step, max_distance)
    "inside_a_tile_yaw_45_step_100": (_mosaic([(46, 8)]), 46.5, 8.5, 45.0, 100.0, 6000.0),
    "inside_a_tile_step_1": (_mosaic([(46, 8)]), 46.5, 8.5, 45.0, 1.0, 60.0),
    "on_a_tile_edge_yaw_180": (_mosaic([(45, 8), (46, 8)]), 46.0, 8.5, 180.0, 100.0, 6000.0),
    "on_a_tile_corner_yaw_45": (_mosaic(NINE, n=101), 46.0, 9.0, 45.0, 100.0, 5000.0),
    "outside_the_mosaic_looking_in_step_5km": (_mosaic([(46, 8)]), 46.5, 7.7, 90.0, 5000.0, 150_000.0),
    "missing_tile_step_5km": (_mosaic(NINE, n=101, skip=[(46, 9)]), 46.5, 8.5, 90.0, 5000.0, 200_000.0),
    "two_resolutions_side_by_side": ({(46, 8): _rough(3, 301, 301), (46, 9): _rough(4, 61, 61)}, 46.5, 8.97, 90.0, 100.0, 8000.0),
    "two_resolutions_yaw_180": ({(46, 8): _rough(3, 301, 151), (45, 8): _rough(4, 31, 61)}, 46.02, 8.5, 180.0, 100.0, 8000.0),
    "latitude_80_step_100": (_mosaic([(80, 8), (80, 9)]), 80.5, 8.9, 45.0, 100.0, 6000.0),
    "latitude_80_step_5km": (_mosaic([(80, 8), (80, 9), (80, 10)], n=101), 80.5, 8.9, 90.0, 5000.0, 100_000.0),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_sample_lies_below_its_cell_and_suffix(exe, oracle, tmp_path, name):
    tiles, lat, lon, yaw, step, max_distance = CASES[name]
    r = _run(exe, tmp_path, tiles, lat, lon, yaw, step, max_distance, tilt=-5.0 if "yaw_180" in name else 0.0)
    top = max(1, max(int(p.max()) for p in tiles.values())) + 1
    assert (r["cell"][:, -1] == top).all() and (r["cell"] <= top).all() and (r["cell"] >= 1).all()  # the column of the rays outside the bins
    assert (r["suffix"] == np.maximum.accumulate(r["cell"][::-1], axis=0)[::-1]).all()
    if "step_5km" not in name:
        assert r["stat"]["unbounded"] == 0  # only a box of more than a degree may fall back to the mosaic's top
    _oracle_agrees(oracle, tiles, r["samples"])


def test_a_table_of_global_tops_cannot_pass(exe, oracle, tmp_path):
    """zeros and one 3000 m post, 4 km from the observer at azimuth 45 degrees: 1 m wherever the post is outside the cell's box"""
    n, i0, j0 = 301, 158, 161
    posts = np.zeros((n, n), dtype=np.int16)
    posts[i0, j0] = 3000
    post_lat, post_lon = 46.0 + i0 / (n - 1), 8.0 + j0 / (n - 1)
    r = _run(exe, tmp_path, {(46, 8): posts}, 46.5, 8.5, 45.0, 100.0, 8000.0)
    assert r["stat"]["unbounded"] == 0
    dir0, rel_lo, w = r["layout"]
    rows, bins = r["cell"].shape[0], r["cell"].shape[1] - 1
    earth = _abi.EarthModel()
    earth.kind, earth.radius = _abi.EARTH_KINDS["Spherical"], RADIUS
    edges = [oracle.coords_at_dist(earth, 46.5, 8.5, math.degrees(dir0 + rel_lo + j * w), r["xs"]) for j in range(bins + 1)]
    two_posts = 2.0 / (n - 1)
    holds = 0
    for i in range(rows):
        sagitta = r["xs"][i] * (1.0 - math.cos(w / 2)) / (RADIUS * math.pi / 180.0)
        for j in range(bins):
            (la0, lo0), (la1, lo1) = edges[j][i], edges[j + 1][i]
            dlat = sagitta + two_posts
            dlon = sagitta / math.cos(math.radians(max(abs(la0), abs(la1)))) + two_posts
            inside = min(la0, la1) - dlat <= post_lat <= max(la0, la1) + dlat and min(lo0, lo1) - dlon <= post_lon <= max(lo0, lo1) + dlon
            holds += inside
            if not inside:
                assert r["cell"][i, j] == 1.0, (i, j, r["cell"][i, j])
    # the post's own box of two posts (2 x 370 m) is seen from 4 km: it spans every bin of some fifteen rows, a sixth of the table
    assert 0 < (r["cell"][:, :bins] == 3001.0).sum() <= holds < 0.25 * rows * bins


def test_the_cover_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    exe = _exe("ceiling_host_asan_ubsan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    tiles, lat, lon, yaw, step, max_distance = CASES["missing_tile_step_5km"]
    _run(exe, tmp_path, tiles, lat, lon, yaw, step, max_distance)
    tiles, lat, lon, yaw, step, max_distance = CASES["on_a_tile_edge_yaw_180"]
    _run(exe, tmp_path, tiles, lat, lon, yaw, step, max_distance, tilt=-5.0)
