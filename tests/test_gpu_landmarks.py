"""atmrt_locate_landmarks* on the GPU against tests/landmarks_model.py: the model searches the arrays atmrt_generate returned for
the same frame by brute force, and every field of every record (doubles by their bits) and n_points, n_skipped, n_within must agree;
n_tested depends on the library's filter and is only bounded.  A second call must return the same bytes.

Every case prints its figures before it asserts (`landmarks <case> <mode> <set> <radius>: found, statistics`)."""
import ctypes as C
import csv
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import landmarks_model as lm
import visibility_model as vm
from atm_raytracer_amd import _abi, generators, synth
from util import run_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARCSEC = 1.0 / 3600.0
OBSERVER = (46.5, 8.5)  # of scene S2; max_distance 60 km is 0.54 degrees of latitude


def scene(generator, w, h, **over):
    over.setdefault("max_distance", 60_000.0)
    return synth.scene("S2", w, h, generator=generator, **over)


def check(ctx, res, marks, radius, mode, tag, planes=None):
    """One call against the model, a second call against the first.  -> (records, stats)"""
    got, stats = generators.locate_landmarks(ctx, marks, radius, mode, planes=planes)
    want, w_stats = lm.locate(res, marks, radius, mode)
    print(f"landmarks {tag} {mode} r={radius / ARCSEC:g}as: {len(marks)} landmarks, {int((got['n_within'] > 0).sum())} found "
          f"(model {int((want['n_within'] > 0).sum())}), largest n_within {int(got['n_within'].max())}, {stats}, model {w_stats}")
    lm.assert_records(got, want, tag)
    for k in ("n_points", "n_skipped", "n_within"):
        assert stats[k] == w_stats[k], (tag, k, stats, w_stats)
    assert stats["n_tested"] >= stats["n_within"] == int(got["n_within"].astype(np.int64).sum()), (tag, stats)
    again, stats2 = generators.locate_landmarks(ctx, marks, radius, mode, planes=planes)
    assert again.tobytes() == got.tobytes() and stats2 == stats, tag
    return got, stats


def landmark_sets(res, mode, rng):
    """Landmarks made from the frame itself: name -> (lat, lon)."""
    lat, lon, dist, pixel = vm.points(res, mode)
    keep = np.flatnonzero(~vm.skipped(lat, lon, dist))
    assert keep.size > 200
    b = vm.bounds(lat, lon, dist)
    pick = keep[np.unique(np.r_[0, keep.size - 1, rng.integers(0, keep.size, 10)])]
    a = keep[rng.integers(0, keep.size - 1, 8)]
    c = keep[np.minimum(np.searchsorted(keep, a) + 1, keep.size - 1)]  # the next point in pixel order: mostly the neighbouring pixel
    mid_lat, mid_lon = 0.5 * (lat[a] + lat[c]), 0.5 * (lon[a] + lon[c])
    outside_lat = np.array([b[1] + 2.0, b[0] - 2.0, 0.5 * (b[0] + b[1]), 0.5 * (b[0] + b[1])])
    outside_lon = np.array([0.5 * (b[2] + b[3]), 0.5 * (b[2] + b[3]), b[3] + 3.0, b[2] - 3.0])
    return {
        # exact trace points (d2 = 0: the tie order decides), midpoints, the first exact point twice more, and well outside
        "mixed": (np.r_[lat[pick], mid_lat, lat[pick[0]], lat[pick[0]], outside_lat], np.r_[lon[pick], mid_lon, lon[pick[0]], lon[pick[0]], outside_lon]),
        "one": (lat[pick[1:2]], lon[pick[1:2]]),
        "uniform": (rng.uniform(b[0], b[1], 5000), rng.uniform(b[2], b[3], 5000)),
        "wide": (OBSERVER[0] + rng.uniform(-0.01, 0.01, 16), OBSERVER[1] + rng.uniform(-0.01, 0.01, 16)),
    }


def check_frame(ctx, res, name, modes=("first", "all")):
    rng = np.random.default_rng(sorted(FRAMES).index(name) if name in FRAMES else 99)
    for mode in modes:
        sets = landmark_sets(res, mode, rng)
        n_valid = None
        for set_name, radii in (("mixed", (1 * ARCSEC, 30 * ARCSEC)), ("one", (30 * ARCSEC,)), ("uniform", (1 * ARCSEC, 30 * ARCSEC)), ("wide", (1.0,))):
            if mode == "all" and set_name == "uniform" and modes != ("all",) and name != "translucent":
                continue  # ALL on a frame without lists is FIRST: the small sets show it
            marks = generators.landmarks(*sets[set_name])
            for radius in radii:
                got, stats = check(ctx, res, marks, radius, mode, f"{name} {set_name}")
                n_valid = stats["n_points"] - stats["n_skipped"]
                if set_name == "mixed":
                    n = len(marks)
                    assert (got["n_within"][:n - 14] > 0).all() and (got["d2"][:n - 14] == 0).all()  # an exact point finds itself, or an equal one
                    assert got[n - 6] == got[n - 5] == got[0]  # equal landmarks, equal records
                    assert not got["n_within"][n - 4:].any()  # well outside
                if set_name == "one":
                    assert got["n_within"][0] >= 1 and got["d2"][0] == 0
                if set_name == "wide":  # every point is within every landmark: long lists, all lanes contend
                    assert (got["n_within"] == n_valid).all() and stats["n_within"] == 16 * n_valid == stats["n_tested"]


FRAMES = {
    "fast": dict(generator="Fast", w=96, h=48, over=dict(tilt=-3.0)),
    "rect": dict(generator="Rectilinear", w=96, h=48, over=dict()),
    "interp": dict(generator="InterpolatingRectilinear", w=96, h=48, over=dict()),
    "tail": dict(generator="Fast", w=100, h=37, over=dict(tilt=-3.0)),  # 3700 pixels: 52 tail lanes, a tail block of 116 threads
}


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_opaque_frames(gpu_ctx, name):
    c = FRAMES[name]
    cfg, tiles = scene(c["generator"], c["w"], c["h"], **c["over"])
    res = run_gpu(gpu_ctx, cfg, tiles)
    assert res["n_hits"] > c["w"] * c["h"] // 4
    check_frame(gpu_ctx, res, name)


def test_column_shard_counts_from_its_own_first_column(gpu_ctx):
    cfg, tiles = scene("Fast", 128, 48, tilt=-3.0)
    cfg.params.col_begin, cfg.params.col_end = 32, 100
    res = run_gpu(gpu_ctx, cfg, tiles)
    assert res["hit_count"].shape == (48, 68)
    check_frame(gpu_ctx, res, "shard")
    lat, lon, dist, pixel = vm.points(res, "first")
    last = np.flatnonzero(~vm.skipped(lat, lon, dist))[-1]
    got, _ = generators.locate_landmarks(gpu_ctx, generators.landmarks(lat[last:last + 1], lon[last:last + 1]), 1 * ARCSEC)
    assert got["d2"][0] == 0 and got["x"][0] < 68 and got["y"][0] * 68 + got["x"][0] <= pixel[last]


def test_translucent_terrain_all_reads_the_lists(gpu_ctx):
    cfg, tiles = scene("Rectilinear", 64, 48, terrain_alpha=0.5)
    res = run_gpu(gpu_ctx, cfg, tiles)
    assert (res["hit_count"] > 1).any()
    check_frame(gpu_ctx, res, "translucent")
    # a landmark on the LAST point of a pixel with several: ALL finds it at its index, FIRST does not see it
    cnt, off = res["hit_count"].ravel().astype(np.int64), res["hit_offset"].ravel().astype(np.int64)
    p = int(np.flatnonzero(cnt > 1)[0])
    k = off[p] + cnt[p] - 1
    marks = generators.landmarks([res["lat"][k]], [res["lon"][k]])
    every, st_all = check(gpu_ctx, res, marks, 1 * ARCSEC, "all", "translucent last point")
    first, st_first = check(gpu_ctx, res, marks, 1 * ARCSEC, "first", "translucent last point")
    assert every["d2"][0] == 0 and st_all["n_points"] == res["n_hits"] > st_first["n_points"] == int((cnt > 0).sum())
    assert (every["y"][0] * 64 + every["x"][0], every["point"][0]) <= (p, cnt[p] - 1) and first["point"][0] == 0


def frame_planes(res):
    """The frame's own first-point planes as torch tensors: NaN where a pixel has no point."""
    h, w = res["hit_count"].shape
    hit = res["hit_count"] > 0
    first = res["hit_offset"][hit].astype(np.int64)
    planes = {}
    for k in ("lat", "lon", "distance", "elevation"):
        a = np.full((h, w), np.nan)
        a[hit] = res[k][first]
        planes[k] = torch.from_numpy(a).cuda()
    planes["hit_count"] = torch.from_numpy(res["hit_count"].astype(np.int32)).cuda()
    return planes


def test_planes_variant_equals_first_mode(gpu_ctx):
    cfg, tiles = scene("Fast", 100, 37, tilt=-3.0)
    res = run_gpu(gpu_ctx, cfg, tiles)
    planes = frame_planes(res)
    sets = landmark_sets(res, "first", np.random.default_rng(5))
    for set_name, radius in (("mixed", 30 * ARCSEC), ("uniform", 1 * ARCSEC), ("uniform", 30 * ARCSEC), ("wide", 1.0)):
        marks = generators.landmarks(*sets[set_name])
        want, w_stats = generators.locate_landmarks(gpu_ctx, marks, radius, "first")
        got, stats = check(gpu_ctx, res, marks, radius, "first", f"planes {set_name}", planes=planes)
        assert got.tobytes() == want.tobytes() and stats == w_stats


def test_hand_made_planes(gpu_ctx):
    """What no generated frame guarantees: NaN, -0.0, negative and infinite distances; points exactly on the radius and one ulp beyond
    it; exact ties in different rows."""
    u, w, h = 1.0 / 1024, 70, 5
    rng = np.random.default_rng(21)
    lat = 47.0 + rng.integers(-40, 41, (h, w)) * u  # a lattice of exactly representable coordinates: many exact ties
    lon = 8.0 + rng.integers(-40, 41, (h, w)) * u
    dist = rng.uniform(10.0, 1000.0, (h, w))
    elev = rng.uniform(-10.0, 4000.0, (h, w))
    cnt = np.ones((h, w), dtype=np.uint32)
    # row 0: the 3-4-5 points around (47, 8), on the radius 5 u and one ulp beyond it in either coordinate
    sgn = [(1, 1), (1, -1), (-1, 1), (-1, -1)]
    for i, (a, b) in enumerate(sgn):
        lat[0, i], lon[0, i] = 47.0 + a * 3 * u, 8.0 + b * 4 * u
        lat[0, 4 + i], lon[0, 4 + i] = np.nextafter(47.0 + a * 3 * u, 47.0 + a), 8.0 + b * 4 * u
        lat[0, 8 + i], lon[0, 8 + i] = 47.0 + a * 3 * u, np.nextafter(8.0 + b * 4 * u, 8.0 + b)
    # the same point in rows 1, 2 and 4 (x = 69, 3, 3): the smallest flat index wins; row 3 holds it too, but is skipped
    for y, x in ((1, 69), (2, 3), (3, 0), (4, 3)):
        lat[y, x], lon[y, x] = 47.0 + 100 * u, 8.0 + 100 * u
    dist[3, 0] = np.nan
    lat[1, 10], lon[1, 11], dist[1, 12] = np.nan, np.nan, np.nan
    dist[2, 20], dist[2, 21], dist[2, 22], dist[2, 23], dist[2, 24] = -1.0, -0.0, 0.0, np.inf, -np.inf
    lat[2, 20:25], lon[2, 20:25] = 47.0 + (200 + 20 * np.arange(5)) * u, 8.0 + 200 * u  # places of their own, farther apart than the radius
    lat[4, 30], lon[4, 31] = np.inf, -np.inf
    cnt[3, 40:50], cnt[4, 60] = 0, 5
    lat[3, 40:50], lon[3, 40:50] = 47.0, 8.0  # no point there, whatever the planes say
    planes = {"lat": torch.from_numpy(lat).cuda(), "lon": torch.from_numpy(lon).cuda(), "distance": torch.from_numpy(dist).cuda(),
              "elevation": torch.from_numpy(elev).cuda(), "hit_count": torch.from_numpy(cnt.astype(np.int32)).cuda()}
    res = lm.hand_made(lat, lon, dist, elev, cnt)
    l_lat = np.r_[47.0, 47.0, 47.0 + 100 * u, lat[2, 20:25], rng.integers(-40, 41, 40) * u + 47.0, 47.0 + 0.5 * u]
    l_lon = np.r_[8.0, 8.0, 8.0 + 100 * u, lon[2, 20:25], rng.integers(-40, 41, 40) * u + 8.0, 8.0 + 0.5 * u]
    marks = generators.landmarks(l_lat, l_lon, 1.0)
    got, stats = check(gpu_ctx, res, marks, 5 * u, "first", "hand-made", planes=planes)
    assert stats["n_points"] == h * w - 10 and stats["n_skipped"] == 6  # 4 NaN, -1.0, -inf; lat / lon = +-inf are looked up, never within
    on_radius = lm.within(47.0, 8.0, 1.0, lat[0, :12], lon[0, :12], 5 * u)
    assert on_radius.tolist() == [True] * 4 + [False] * 8
    assert got[0] == got[1] and got["n_within"][0] >= 4
    assert got["n_within"][2] == 3 and (got["x"][2], got["y"][2], got["d2"][2]) == (69, 1, 0.0)
    assert got["n_within"][3] == 0 and got["n_within"][7] == 0  # the points with distance -1.0 and -inf are skipped
    assert (got["x"][4], got["y"][4], got["d2"][4]) == (21, 2, 0.0) and np.signbit(got["distance"][4])  # -0.0: its bits as the frame holds them
    assert (got["x"][6], got["y"][6]) == (23, 2) and np.isposinf(got["distance"][6])
    # a radius so small that its square underflows: only d2 == 0 is within
    tiny, _ = check(gpu_ctx, res, marks, 1e-200, "first", "hand-made tiny radius", planes=planes)
    assert tiny["n_within"][2] == 3 and (tiny["d2"][tiny["n_within"] > 0] == 0).all()
    # the same planes with lon_scale 0.5: (3 u, 8 u * 0.5) is on the radius
    lon2 = lon.copy()
    lon2[0, :12] = 8.0 + (lon[0, :12] - 8.0) * 2.0
    planes["lon"] = torch.from_numpy(lon2).cuda()
    check(gpu_ctx, lm.hand_made(lat, lon2, dist, elev, cnt), generators.landmarks(l_lat, l_lon, 0.5), 5 * u, "first", "hand-made half scale", planes=planes)


def test_state_and_argument_errors(gpu_ctx):
    lib = gpu_ctx.lib
    marks = generators.landmarks([46.6, 46.7], [8.5, 8.6])
    hits = np.zeros(2, dtype=generators.LANDMARK_HIT_DTYPE)
    st = _abi.LandmarkStats()
    call = lambda c, m=marks, n=2, r=3 * ARCSEC, mode=0, out=hits: lib.atmrt_locate_landmarks(c.handle, m, n, r, mode, out.ctypes.data if out is not None else None,
                                                                                              C.byref(st))
    fresh = generators.Context(0)
    try:
        assert call(fresh) == _abi.ERR_STATE and b"needs a frame" in lib.atmrt_last_error(fresh.handle)
        cfg, tiles = scene("Fast", 96, 48, tilt=-3.0)
        res = run_gpu(fresh, cfg, tiles)
        assert call(fresh) == 0 and st.n_points == int((res["hit_count"] > 0).sum())
        assert lib.atmrt_locate_landmarks(fresh.handle, marks, 2, 3 * ARCSEC, 1, hits.ctypes.data, None) == 0  # stats may be NULL
        good = hits.copy()
        for kw in (dict(n=0), dict(n=(1 << 20) + 1), dict(m=None), dict(out=None), dict(r=0.0), dict(r=-1.0), dict(r=float("nan")), dict(r=float("inf")),
                   dict(r=1.5), dict(mode=2), dict(mode=-1)):
            assert call(fresh, **kw) == _abi.ERR_INVALID_ARGUMENT and lib.atmrt_last_error(fresh.handle), kw
        for field, value in (("lat", float("nan")), ("lon", float("inf")), ("lon_scale", 0.0), ("lon_scale", 1.5), ("lon_scale", float("nan"))):
            bad = generators.landmarks([46.6, 46.7], [8.5, 8.6])
            setattr(bad[1], field, value)
            assert call(fresh, m=bad) == _abi.ERR_INVALID_ARGUMENT and b"landmark" in lib.atmrt_last_error(fresh.handle), (field, value)
        assert hits.tobytes() == good.tobytes()
        d = torch.zeros((4, 4), dtype=torch.float64, device="cuda")
        d_cnt = torch.zeros((4, 4), dtype=torch.int32, device="cuda")
        planes = lambda **kw: lib.atmrt_locate_landmarks_planes_device(fresh.handle, marks, 2, 3 * ARCSEC, kw.get("lat", d.data_ptr()), d.data_ptr(), d.data_ptr(),
                                                                       kw.get("elev", d.data_ptr()), kw.get("cnt", d_cnt.data_ptr()), 4, 4, hits.ctypes.data, None)
        assert planes() == 0 and not hits["n_within"].any()
        for null in ("lat", "elev", "cnt"):
            assert planes(**{null: None}) == _abi.ERR_INVALID_ARGUMENT and b"plane" in lib.atmrt_last_error(fresh.handle)
        # after a failed frame the frame before it is gone, and the next good frame is searched again
        assert lib.atmrt_debug_fail_next_frame(fresh.handle) == 0
        with pytest.raises(generators.AtmrtError):
            run_gpu(fresh, cfg, tiles)
        assert call(fresh) == _abi.ERR_STATE
        run_gpu(fresh, cfg, tiles)
        assert call(fresh) == 0 and hits.tobytes() == good.tobytes()
    finally:
        fresh.close()


def test_multi_device_context_takes_the_planes_route(gpu_ctx):
    cfg, tiles = scene("Fast", 90, 40, tilt=-3.0)
    res = run_gpu(gpu_ctx, cfg, tiles)
    sets = landmark_sets(res, "first", np.random.default_rng(8))
    marks = generators.landmarks(*sets["mixed"])
    single, s_stats = generators.locate_landmarks(gpu_ctx, marks, 30 * ARCSEC)
    ctx = generators.Context.multi([0, 0])
    try:
        gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
        dev = torch.device("cuda", 0)
        images = [generators.image_planes(40, 90, dev) for _ in range(2)]
        gen.generate_image_device([pod for _, pod in images])
        hits = np.zeros(len(marks), dtype=generators.LANDMARK_HIT_DTYPE)
        assert ctx.lib.atmrt_locate_landmarks(ctx.handle, marks, len(marks), 30 * ARCSEC, 0, hits.ctypes.data, None) == _abi.ERR_STATE
        assert b"atmrt_locate_landmarks_planes_device" in ctx.lib.atmrt_last_error(ctx.handle)
        got, stats = generators.locate_landmarks(ctx, marks, 30 * ARCSEC, planes=images[-1][0])
        print(f"landmarks gathered: {stats}, single {s_stats}")
        lm.assert_records(got, single, "gathered")
        assert {k: stats[k] for k in ("n_points", "n_skipped", "n_within")} == {k: s_stats[k] for k in ("n_points", "n_skipped", "n_within")}
    finally:
        ctx.close()


def test_cli_gen_writes_the_table(tmp_path, gpu_ctx):
    from atm_raytracer_amd import config
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Relative": 50.0}},
                    "frame": {"direction": 40.0, "fov": 30.0, "tilt": -2.0, "max_distance": 60000.0}},
           "simulation_step": 100.0, "output": {"width": 96, "height": 48, "generator": "Fast"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    # the same frame through the library, to pick landmarks that are in it
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    res = generators.make_generator(generators.Params(cfg), terrain).generate()
    lat, lon, dist, _ = vm.points(res, "first")
    keep = np.flatnonzero(~vm.skipped(lat, lon, dist))
    pick = keep[[0, keep.size // 3, keep.size // 2, keep.size - 1]]
    names = ["first", "third, quoted", "half", "last", "nowhere"]
    l_lat, l_lon = np.r_[lat[pick], 10.0], np.r_[lon[pick] + 2 * ARCSEC, 10.0]
    with open(tmp_path / "peaks.csv", "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["name", "lat", "lon"])
        for row in zip(names, l_lat.tolist(), l_lon.tolist()):
            w.writerow([row[0], repr(row[1]), repr(row[2])])
    r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", "out.png", "--landmarks", "peaks.csv",
                        "--landmark-radius", "30", "--landmarks-out", "found.csv"], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert (tmp_path / "out.png").exists()
    with open(tmp_path / "found.csv", newline="") as f:
        rows = list(csv.reader(f))
    assert tuple(rows[0]) == generators.LANDMARK_COLUMNS and len(rows) == 6
    want, _ = lm.locate(res, generators.landmarks(l_lat, l_lon), 30 * ARCSEC, "first")
    print("landmarks cli:", rows[1:], want)
    for row, name, a, b, h in zip(rows[1:], names, l_lat.tolist(), l_lon.tolist(), want):
        assert row[:3] == [name, repr(a), repr(b)] and int(row[3]) == int(h["n_within"] > 0) and int(row[10]) == h["n_within"]
        if h["n_within"]:
            assert (int(row[4]), int(row[5]), int(row[6])) == (h["x"], h["y"], h["point"])
            assert float(row[7]) == float(np.sqrt(h["d2"]) * 3600.0) and float(row[8]) == h["distance"] and float(row[9]) == h["elevation"]
        else:
            assert row[4:10] == [""] * 6
    assert want["n_within"][:4].all() and want["n_within"][4] == 0
