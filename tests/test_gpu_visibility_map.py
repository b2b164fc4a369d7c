"""atmrt_visibility_map* and atmrt_frame_bounds on the GPU against tests/visibility_model.py: the model bins the arrays atmrt_generate
returned for the same frame (np.add.at / np.minimum.at), and every count, every min_distance bit and every statistic must agree.

Every case prints its figures before it asserts (`vis <case> <mode> <grid>: cells, statistics, the model's run count`)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import yaml

import visibility_model as vm
from atm_raytracer_amd import _abi, config, generators, synth
from util import bits, run_gpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE_CELL = _abi.GeoGrid(-90.0, -180.0, 180.0, 360.0, 1, 1)


def scene(generator, w, h, **over):
    over.setdefault("max_distance", 60_000.0)
    return synth.scene("S2", w, h, generator=generator, **over)


def grids_of(b):
    """One cell over everything; 2 x 2 cells whose south-west corner is the centre of the frame's bounds; 1-arcsecond cells."""
    lat_mid, lon_mid = 0.5 * (b[0] + b[1]), 0.5 * (b[2] + b[3])
    quarter = _abi.GeoGrid(lat_mid, lon_mid, max(b[1] - b[0], 1e-6) / 5.0, max(b[3] - b[2], 1e-6) / 5.0, 2, 2)
    return {"one": ONE_CELL, "2x2": quarter, "1as": generators.snap_grid(b, 1.0 / 3600.0)}


def map_numpy(ctx, grid, mode):
    count, mind, stats = generators.visibility_map_device(ctx, grid, mode)
    return count.cpu().numpy().view(np.uint32), mind.cpu().numpy(), stats


def assert_map(got, want, tag):
    (g_count, g_min, g_stats), (w_count, w_min, w_stats) = got, want
    assert g_count.shape == w_count.shape and g_count.dtype == np.uint32, tag
    bad = np.flatnonzero(g_count.ravel() != w_count.ravel())
    assert bad.size == 0, (tag, bad.size, bad[:5], g_count.ravel()[bad[:5]], w_count.ravel()[bad[:5]])
    bad = np.flatnonzero(bits(g_min).ravel() != bits(w_min).ravel())
    assert bad.size == 0, (tag, bad.size, bad[:5], g_min.ravel()[bad[:5]], w_min.ravel()[bad[:5]])
    for k in ("n_points", "n_binned", "n_outside", "n_skipped"):
        assert g_stats[k] == w_stats[k], (tag, k, g_stats, w_stats)


def aggregate_off():
    class Off:
        def __enter__(self):
            self.before = os.environ.get("ATMRT_VIS_AGGREGATE")
            os.environ["ATMRT_VIS_AGGREGATE"] = "off"

        def __exit__(self, *exc):
            if self.before is None:
                del os.environ["ATMRT_VIS_AGGREGATE"]
            else:
                os.environ["ATMRT_VIS_AGGREGATE"] = self.before
    return Off()


def check_frame(ctx, res, name, modes=("first", "all")):
    """Every requirement of a case, for the frame `res` that is the last one on ctx.  -> {(mode, grid name): stats}."""
    out = {}
    n_waves = (res["hit_count"].size + vm.WAVE - 1) // vm.WAVE
    for mode in modes:
        lat, lon, dist, _ = vm.points(res, mode)
        want_b = vm.bounds(lat, lon, dist)
        got_b = generators.frame_bounds(ctx, mode)
        assert np.array_equal(bits(np.array(got_b)), bits(np.array(want_b))), (name, mode, got_b, want_b)
        for gname, grid in grids_of(want_b).items():
            tag = (name, mode, gname)
            want = vm.model_map(grid, lat, lon, dist)
            got = map_numpy(ctx, grid, mode)
            assert_map(got, want, tag)
            stats = got[2]
            runs = vm.first_mode_runs(grid, res) if mode == "first" else None
            print(f"vis {name} {mode} {gname}: {grid.n_lat}x{grid.n_lon} cells, {stats}, model runs {runs}, wavefronts {n_waves}")
            assert stats["n_updates"] <= stats["n_binned"]
            if mode == "first":
                assert stats["n_updates"] <= runs, tag
            host = generators.visibility_map(ctx, grid, mode)  # the host-array variant
            assert_map(host, got, tag)
            assert host[2]["n_updates"] == stats["n_updates"]
            with aggregate_off():
                plain = map_numpy(ctx, grid, mode)
            assert_map(plain, got, tag)
            assert plain[2]["n_updates"] == plain[2]["n_binned"], tag
            if gname == "one":
                assert got[0][0, 0] == stats["n_binned"] == stats["n_points"] - stats["n_skipped"] and stats["n_outside"] == 0
                # a wavefront is 64 consecutive pixels of at most two image rows (every frame here is wider than 64): the pixels of a
                # row that see ground are one run unless sky shows between them, so a wavefront issues a few updates, not 64
                # (FIRST mode: the later trips of ALL mode see only the scattered pixels that have further points)
                if mode == "first":
                    assert stats["n_updates"] <= 4 * n_waves, tag
            if gname == "2x2":
                assert stats["n_outside"] > 0 and stats["n_binned"] > 0, tag
            if gname == "1as":
                assert (got[0] <= 1).sum() > got[0].size // 2, tag  # most cells hold at most one point
                assert stats["n_outside"] == 0, tag
            out[(mode, gname)] = stats
    return out


OPAQUE = {
    "fast": dict(generator="Fast", w=96, h=48, over=dict(tilt=-3.0)),
    "rect": dict(generator="Rectilinear", w=96, h=48, over=dict()),
    "interp": dict(generator="InterpolatingRectilinear", w=96, h=48, over=dict()),
    "tail": dict(generator="Fast", w=100, h=37, over=dict(tilt=-3.0)),  # 3700 pixels: 52 tail lanes, a tail block of 116 threads
}


@pytest.mark.parametrize("name", sorted(OPAQUE))
def test_opaque_frames(gpu_ctx, name):
    c = OPAQUE[name]
    cfg, tiles = scene(c["generator"], c["w"], c["h"], **c["over"])
    res = run_gpu(gpu_ctx, cfg, tiles)
    assert res["n_hits"] > c["w"] * c["h"] // 4
    stats = check_frame(gpu_ctx, res, name)
    assert stats[("all", "one")]["n_points"] == stats[("first", "one")]["n_points"] == int((res["hit_count"] > 0).sum())


def test_column_shard_is_a_frame_of_its_own(gpu_ctx):
    cfg, tiles = scene("Fast", 128, 48, tilt=-3.0)
    cfg.params.col_begin, cfg.params.col_end = 32, 100
    res = run_gpu(gpu_ctx, cfg, tiles)
    assert res["hit_count"].shape == (48, 68)
    check_frame(gpu_ctx, res, "shard")


def test_translucent_terrain_all_reads_the_lists(gpu_ctx):
    cfg, tiles = scene("Rectilinear", 64, 48, terrain_alpha=0.5)
    res = run_gpu(gpu_ctx, cfg, tiles)
    assert (res["hit_count"] > 1).any()
    stats = check_frame(gpu_ctx, res, "translucent")
    n_first, n_all = stats[("first", "one")]["n_points"], stats[("all", "one")]["n_points"]
    assert n_first == int((res["hit_count"] > 0).sum()) and n_all == res["n_hits"] and n_all > n_first


def test_object_points_are_binned_like_any_other(gpu_ctx):
    cfg, tiles = scene("Fast", 96, 48, tilt=-3.0)
    synth.add_objects(cfg, n_cyl=8, n_bill=0, dist=(800.0, 6_000.0), spread_deg=25.0, radius=(60.0, 150.0), height=(300.0, 800.0))
    res = run_gpu(gpu_ctx, cfg, tiles)
    assert (res["color_tag"] == _abi.COLOR_RGBA).any(), "no pixel of the frame sees an object"
    stats = check_frame(gpu_ctx, res, "objects", modes=("all",))
    assert stats[("all", "one")]["n_points"] == res["n_hits"]


def test_a_frame_of_sky(gpu_ctx):
    cfg, tiles = scene("Fast", 96, 48, tilt=60.0)
    res = run_gpu(gpu_ctx, cfg, tiles)
    assert res["n_hits"] == 0
    grid = _abi.GeoGrid(46.0, 8.0, 0.125, 0.125, 8, 8)
    for mode in ("first", "all"):
        assert all(np.isnan(b) for b in generators.frame_bounds(gpu_ctx, mode))
        for variant in (map_numpy, generators.visibility_map):
            count, mind, stats = variant(gpu_ctx, grid, mode)
            assert not count.any() and np.isposinf(mind).all() and count.shape == (8, 8)
            assert stats == {"n_points": 0, "n_binned": 0, "n_outside": 0, "n_skipped": 0, "n_updates": 0}


def test_planes_variant_equals_the_context_variant(gpu_ctx):
    cfg, tiles = scene("Fast", 100, 37, tilt=-3.0)
    res = run_gpu(gpu_ctx, cfg, tiles)
    h, w = res["hit_count"].shape
    hit = res["hit_count"] > 0
    first = res["hit_offset"][hit].astype(np.int64)
    planes = {}
    for k in ("lat", "lon", "distance"):  # the frame's own planes: the first trace point, NaN where there is none
        a = np.full((h, w), np.nan)
        a[hit] = res[k][first]
        planes[k] = torch.from_numpy(a).cuda()
    planes["hit_count"] = torch.from_numpy(res["hit_count"].astype(np.int32)).cuda()
    lat, lon, dist, _ = vm.points(res, "first")
    for gname, grid in grids_of(vm.bounds(lat, lon, dist)).items():
        want = map_numpy(gpu_ctx, grid, "first")
        count, mind, stats = generators.visibility_map_device(gpu_ctx, grid, "first", planes=planes)
        assert_map((count.cpu().numpy().view(np.uint32), mind.cpu().numpy(), stats), want, gname)
        assert stats["n_updates"] == want[2]["n_updates"]
        # without min_distance: the counts alone
        count2 = torch.full((grid.n_lat, grid.n_lon), 7, dtype=torch.int32, device="cuda")
        gpu_ctx.check(gpu_ctx.lib.atmrt_visibility_map_device(gpu_ctx.handle, C.byref(grid), _abi.VIS_FIRST, count2.data_ptr(), None, None))
        assert torch.equal(count2, count)


def test_skipped_points_of_explicit_planes(gpu_ctx):
    """NaN and negative points are skipped and counted, -0.0 is a distance of 0.0, hit_count == 0 is no point: planes that say so."""
    w, h = 70, 3
    rng = np.random.default_rng(11)
    lat = 46.0 + np.repeat(rng.integers(0, 4, (h, w // 14)), 14, axis=1) * 0.25 + 0.1
    lon = 8.0 + np.repeat(rng.integers(0, 4, (h, w // 7)), 7, axis=1) * 0.25 + 0.1  # runs of 7 equal columns
    dist = rng.uniform(10.0, 1000.0, (h, w))
    cnt = np.ones((h, w), dtype=np.uint32)
    lat[0, 3], lon[0, 9], dist[0, 12] = np.nan, np.nan, np.nan
    dist[1, 5], dist[1, 6], dist[2, 7] = -1.0, -0.0, 0.0
    cnt[2, 20:30], cnt[1, 40] = 0, 5
    lat[2, 64:] = 99.0  # outside
    grid = _abi.GeoGrid(46.0, 8.0, 0.25, 0.25, 4, 4)
    planes = {"lat": torch.from_numpy(lat).cuda(), "lon": torch.from_numpy(lon).cuda(), "distance": torch.from_numpy(dist).cuda(),
              "hit_count": torch.from_numpy(cnt.astype(np.int32)).cuda()}
    res = {"hit_count": np.minimum(cnt, 1), "hit_offset": np.arange(h * w).reshape(h, w), "lat": lat.ravel(), "lon": lon.ravel(),
           "distance": dist.ravel()}
    p_lat, p_lon, p_dist, _ = vm.points(res, "first")
    want = vm.model_map(grid, p_lat, p_lon, p_dist)
    assert want[2] == {"n_points": h * w - 10, "n_binned": h * w - 10 - 4 - 6, "n_outside": 6, "n_skipped": 4}
    assert want[1].min() == 0.0 and not np.signbit(want[1].min())
    for off in (False, True):
        if off:
            with aggregate_off():
                count, mind, stats = generators.visibility_map_device(gpu_ctx, grid, "first", planes=planes)
        else:
            count, mind, stats = generators.visibility_map_device(gpu_ctx, grid, "first", planes=planes)
        assert_map((count.cpu().numpy().view(np.uint32), mind.cpu().numpy(), stats), want, off)
        assert stats["n_updates"] == stats["n_binned"] if off else stats["n_updates"] <= vm.first_mode_runs(grid, res) < stats["n_binned"]


def test_state_and_argument_errors(gpu_ctx):
    lib = gpu_ctx.lib
    grid = _abi.GeoGrid(46.0, 8.0, 0.125, 0.125, 8, 8)
    count, mind = np.zeros((8, 8), dtype=np.uint32), np.zeros((8, 8))
    d_count = torch.zeros((8, 8), dtype=torch.int32, device="cuda")
    d_min = torch.zeros((8, 8), dtype=torch.float64, device="cuda")
    st = _abi.VisibilityStats()
    b = (C.c_double * 4)()
    host = lambda c, g=grid, mode=0, cnt=count: lib.atmrt_visibility_map(c.handle, C.byref(g), mode, cnt.ctypes.data if cnt is not None else None,
                                                                         mind.ctypes.data, C.byref(st))
    dev = lambda c, g=grid, mode=0, cnt=d_count: lib.atmrt_visibility_map_device(c.handle, C.byref(g), mode, cnt.data_ptr() if cnt is not None else None,
                                                                                 d_min.data_ptr(), C.byref(st))
    fresh = generators.Context(0)
    try:
        for call in (host, dev):
            assert call(fresh) == _abi.ERR_STATE and b"needs a frame" in lib.atmrt_last_error(fresh.handle)
        assert lib.atmrt_frame_bounds(fresh.handle, 0, b) == _abi.ERR_STATE
        cfg, tiles = scene("Fast", 96, 48, tilt=-3.0)
        res = run_gpu(fresh, cfg, tiles)
        assert host(fresh) == 0 and dev(fresh) == 0 and lib.atmrt_frame_bounds(fresh.handle, 1, b) == 0
        good = count.copy()
        assert good.sum() == st.n_binned > 0
        # every bad grid, an unknown mode, NULL pointers: refused with a message, nothing written
        from test_visibility_abi import bad_grids
        for bad in bad_grids():
            for call in (host, dev):
                assert call(fresh, g=bad) == _abi.ERR_INVALID_ARGUMENT and b"grid" in lib.atmrt_last_error(fresh.handle)
            rc = lib.atmrt_visibility_map_planes_device(fresh.handle, C.byref(bad), d_min.data_ptr(), d_min.data_ptr(), d_min.data_ptr(),
                                                        d_count.data_ptr(), 8, 8, d_count.data_ptr(), d_min.data_ptr(), None)
            assert rc == _abi.ERR_INVALID_ARGUMENT
        for mode in (2, -1):
            for call in (host, dev):
                assert call(fresh, mode=mode) == _abi.ERR_INVALID_ARGUMENT and b"mode" in lib.atmrt_last_error(fresh.handle)
            assert lib.atmrt_frame_bounds(fresh.handle, mode, b) == _abi.ERR_INVALID_ARGUMENT
        for call in (host, dev):
            assert call(fresh, cnt=None) == _abi.ERR_INVALID_ARGUMENT and b"count" in lib.atmrt_last_error(fresh.handle)
        assert lib.atmrt_visibility_map(fresh.handle, None, 0, count.ctypes.data, None, None) == _abi.ERR_INVALID_ARGUMENT
        assert lib.atmrt_visibility_map_planes_device(fresh.handle, C.byref(grid), None, d_min.data_ptr(), d_min.data_ptr(), d_count.data_ptr(), 8, 8,
                                                      d_count.data_ptr(), None, None) == _abi.ERR_INVALID_ARGUMENT
        assert lib.atmrt_frame_bounds(fresh.handle, 0, None) == _abi.ERR_INVALID_ARGUMENT
        assert np.array_equal(count, good)
        # after a failed frame the planes of the frame before it are gone ...
        assert lib.atmrt_debug_fail_next_frame(fresh.handle) == 0
        with pytest.raises(generators.AtmrtError):
            run_gpu(fresh, cfg, tiles)
        for call in (host, dev):
            assert call(fresh) == _abi.ERR_STATE
        assert lib.atmrt_frame_bounds(fresh.handle, 0, b) == _abi.ERR_STATE
        # ... and the next good frame has a map again
        res = run_gpu(fresh, cfg, tiles)
        assert host(fresh) == 0 and np.array_equal(count, good)
        lat, lon, dist, _ = vm.points(res, "first")
        assert_map((count, mind, {k: getattr(st, k) for k, _ in _abi.VisibilityStats._fields_}), vm.model_map(grid, lat, lon, dist), "after")
    finally:
        fresh.close()


def test_multi_device_context_names_the_planes_variant(gpu_ctx):
    cfg, tiles = scene("Fast", 90, 40, tilt=-3.0)
    res = run_gpu(gpu_ctx, cfg, tiles)
    lat, lon, dist, _ = vm.points(res, "first")
    grid = grids_of(vm.bounds(lat, lon, dist))["2x2"]
    single = map_numpy(gpu_ctx, grid, "first")
    ctx = generators.Context.multi([0, 0])
    try:
        gen = generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, ctx))
        dev = torch.device("cuda", 0)
        images = [generators.image_planes(40, 90, dev) for _ in range(2)]
        gen.generate_image_device([pod for _, pod in images])
        d_count = torch.zeros((2, 2), dtype=torch.int32, device=dev)
        b = (C.c_double * 4)()
        assert ctx.lib.atmrt_visibility_map_device(ctx.handle, C.byref(grid), 0, d_count.data_ptr(), None, None) == _abi.ERR_STATE
        assert b"atmrt_visibility_map_planes_device" in ctx.lib.atmrt_last_error(ctx.handle)
        assert ctx.lib.atmrt_frame_bounds(ctx.handle, 0, b) == _abi.ERR_STATE
        count, mind, stats = generators.visibility_map_device(ctx, grid, "first", planes=images[-1][0])
        assert_map((count.cpu().numpy().view(np.uint32), mind.cpu().numpy(), stats), single, "gathered")
    finally:
        ctx.close()


def test_cli_gen_writes_the_map(tmp_path, gpu_ctx):
    synth.write_terrain_dir(str(tmp_path / "terrain"), synth.synth_tiles([46], [8], level=301))
    doc = {"scene": {"terrain_folder": "./terrain"},
           "view": {"position": {"latitude": 46.5, "longitude": 8.5, "altitude": {"Relative": 50.0}},
                    "frame": {"direction": 40.0, "fov": 30.0, "tilt": -2.0, "max_distance": 60000.0}},
           "simulation_step": 100.0, "output": {"width": 120, "height": 60, "generator": "Fast"}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(doc))
    r = subprocess.run([sys.executable, "-m", "atm_raytracer_amd", "gen", "-c", "cfg.yaml", "--output", "out.png", "--visibility-map", "m.npz",
                        "--map-cell", "30"], cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = np.load(tmp_path / "m.npz")
    assert {"count", "min_distance", "lat0", "lon0", "cell_lat", "cell_lon", "n_points", "n_binned", "n_outside", "n_skipped", "n_updates"} <= set(m.files)
    assert m["count"].dtype == np.uint32 and m["count"].shape == m["min_distance"].shape and float(m["cell_lat"]) == 30.0 / 3600.0
    # a direct call on the same frame with the same grid
    cfg = config.parse_config(str(tmp_path / "cfg.yaml"))
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))
    terrain = generators.Terrain.from_folder(str(tmp_path / "terrain"), gpu_ctx)
    generators.make_generator(generators.Params(cfg), terrain).generate()
    grid = _abi.GeoGrid(float(m["lat0"]), float(m["lon0"]), float(m["cell_lat"]), float(m["cell_lon"]), *m["count"].shape)
    count, mind, stats = generators.visibility_map(gpu_ctx, grid, "first")
    assert int(m["count"].sum()) == stats["n_binned"] == int(m["n_binned"]) > 0 and stats["n_outside"] == 0
    assert np.array_equal(m["count"], count) and np.array_equal(bits(m["min_distance"]), bits(mind))
