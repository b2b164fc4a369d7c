"""The terrain ceiling table as the DEVICE builds it (k_ceiling_cells / k_ceiling_suffix, csrc/atmrt_kernels.hip), read back through
atmrt_debug_ceiling_table and compared byte for byte with the table tests/csrc/ceiling_host.cpp builds from the same functions —
for every case of tests/test_ceiling_host.py and, on spikes at 3601 posts per degree (tests/ceiling_cases.py), at the shapes where
the two kernels can go wrong: rows around the wavefront's 64 lanes, bins by the hundred and at the cap, atan2's cut inside the
bins.  Then frames marched over that ground, where an entry taken from the neighbouring row or bin loses hits
(tests/test_ceiling_teeth.py proves it on the CPU), against the oracle: opaque and translucent, table on, off and rebuilt, every
march variant (one child process each), three column tiles, two resolutions side by side, objects."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ceiling_cases as cc
import test_ceiling_host as host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    return host._exe("ceiling_host", ["-O2"])


class Resident:
    """One context whose terrain stays in HBM while consecutive frames use the same tiles (a 3601-post tile is 26 MB)."""

    def __init__(self, ctx):
        self.ctx, self.tiles, self.terrain, self.gen = ctx, None, None, None

    def generate(self, cfg, tiles):
        from atm_raytracer_amd import generators
        if self.tiles is not tiles:
            self.ctx.check(self.ctx.lib.atmrt_terrain_clear(self.ctx.handle))
            self.terrain, self.tiles = generators.Terrain.from_tiles(tiles, self.ctx), tiles
        self.gen = generators.make_generator(generators.Params(cfg), self.terrain)
        return self.gen.generate()

    def work(self):
        """(integrated steps, escaped rays, terrain lookups, ceiling_ms) of the last frame"""
        import ctypes as C
        from util import frame_stats
        i, e = C.c_uint64(), C.c_uint64()
        self.ctx.check(self.ctx.lib.atmrt_last_march_work(self.ctx.handle, C.byref(i), C.byref(e)))
        return int(i.value), int(e.value), int(frame_stats(self.ctx)["terrain_lookups"]), self.gen.last_timings()["ceiling_ms"]


@pytest.fixture(scope="module")
def gpu(gpu_ctx):
    r = Resident(gpu_ctx)
    yield r
    gpu_ctx.check(gpu_ctx.lib.atmrt_terrain_clear(gpu_ctx.handle))


class ceiling_mode:
    """ATMRT_CEILING for the frames inside (the library reads it at every frame)"""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.old = os.environ.pop("ATMRT_CEILING", None)
        if self.mode:
            os.environ["ATMRT_CEILING"] = self.mode

    def __exit__(self, *exc):
        os.environ.pop("ATMRT_CEILING", None)
        if self.old is not None:
            os.environ["ATMRT_CEILING"] = self.old


_ORACLE = {}


def _oracle_frame(oracle_det, name):
    """the oracle's frame of cc.marched(name), computed once per session"""
    from util import run_oracle
    if name not in _ORACLE:
        _ORACLE[name] = run_oracle(oracle_det, *cc.marched(name))
    return _ORACLE[name]


# ---- the device table against the host's ----
def _view_config(tiles, lat, lon, yaw, step, reach, tilt=0.0, fov=cc.FOV, generator="Rectilinear", earth_shape=None):
    """a Rectilinear 64 x 32 frame of the host program's view: the same observer, yaw, fov, tilt, step, reach and radius"""
    from atm_raytracer_amd.config import Config
    return Config.from_dict({
        "view": {"position": {"latitude": lat, "longitude": lon, "altitude": {"Absolute": 800.0}},  # (the table does not depend on it)
                 "frame": {"direction": yaw, "fov": fov, "tilt": tilt, "max_distance": reach}},
        "earth_shape": earth_shape or {"Spherical": {"radius": host.RADIUS}}, "straight_rays": False, "simulation_step": step,
        "output": {"width": host.W, "height": host.H, "generator": generator}})


def _assert_table(got, want, tiles):
    """`got`: Context.debug_ceiling_table; `want`: the host program's output.  Layout by its bits, planes byte for byte; and,
    independently of the host, the three properties every table has."""
    rows, stride = want["cell"].shape
    assert (got["rows"], got["n_bins"]) == (rows, stride - 1), (got["rows"], got["n_bins"], rows, stride - 1)
    assert np.array(got["layout"]).tobytes() == np.array(want["layout"]).tobytes(), (got["layout"], want["layout"])
    for plane in ("cell", "suffix"):
        g, w = got[plane], want[plane]
        assert g.shape == w.shape and g.dtype == w.dtype == np.float32
        bad = np.argwhere(g.view(np.uint32) != w.view(np.uint32))
        assert len(bad) == 0, f"{plane}: {len(bad)} of {g.size} entries differ, first (row, bin) {bad[:8].tolist()}: " \
                              f"{[float(g[i, j]) for i, j in bad[:8]]} on the device, {[float(w[i, j]) for i, j in bad[:8]]} on the host"
        assert g.tobytes() == w.tobytes()
    top = max(0, max(int(p.max()) for p in tiles.values())) + 1
    cell, suffix = got["cell"], got["suffix"]
    assert (suffix == np.maximum.accumulate(cell[::-1], axis=0)[::-1]).all()
    assert (cell[:, -1] == top).all() and (suffix[:, -1] == top).all()
    assert (cell >= 1).all() and (cell <= top).all()


def _table_case(gpu, exe, tmp_path, tiles, lat, lon, yaw, step, reach, tilt=0.0, fov=cc.FOV):
    want = host._run(exe, tmp_path, tiles, lat, lon, yaw, step, reach, tilt=tilt, fov=fov, per_cell=-4)
    gpu.generate(_view_config(tiles, lat, lon, yaw, step, reach, tilt, fov), tiles)
    got = gpu.ctx.debug_ceiling_table()
    print(f"\nrows {got['rows']} bins {got['n_bins']}: {int((got['cell'][:, :-1] < got['cell'][0, -1]).sum())} of "
          f"{got['rows'] * got['n_bins']} cells below the mosaic's top, {int((got['suffix'] == 1).sum())} suffix entries of 1 m")
    _assert_table(got, want, tiles)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(host.CASES))
def test_the_device_table_is_the_host_table(gpu, exe, tmp_path, name):
    tiles, lat, lon, yaw, step, reach = host.CASES[name]
    _table_case(gpu, exe, tmp_path, tiles, lat, lon, yaw, step, reach, tilt=-5.0 if "yaw_180" in name else 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["dense", "sparse"])
def test_the_device_table_is_the_host_table_on_spikes(gpu, exe, tmp_path, which):
    got = _table_case(gpu, exe, tmp_path, cc.tile(which), *cc.OBSERVER, cc.YAW, cc.STEP, cc.REACH)
    assert (got["rows"], got["n_bins"]) == (301, 82)
    if which == "sparse":
        assert (got["suffix"][:, :-1] == 1.0).mean() > 0.1  # the last spike of many bins lies inside the reach


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [2, 63, 64, 65, 128, 129, 301])
def test_rows_around_the_suffix_scans_lanes(gpu, exe, tmp_path, rows):
    """k_ceiling_suffix: one wavefront per bin, every lane a run of ceil(rows / 64) steps — 2 rows: 62 empty runs; 64: one step each;
    65: runs of 2, half the lanes empty; 129: runs of 3, the last run short.  2 rows x 82 bins is also a table of less than one
    block of k_ceiling_cells."""
    got = _table_case(gpu, exe, tmp_path, cc.tile("dense"), *cc.OBSERVER, cc.YAW, cc.STEP, (rows - 1) * cc.STEP)
    assert got["rows"] == rows and (rows > 2 or rows * got["n_bins"] < 256)


@pytest.mark.gpu
@pytest.mark.parametrize("name,yaw,tilt,fov,rows", [("fov_120", cc.YAW, 0.0, 120.0, 65), ("fov_120_odd", cc.YAW, 0.0, 120.0, 129),
                                                   ("nadir", cc.YAW, -80.0, 60.0, 65), ("yaw_180", 180.0, 0.0, cc.FOV, 301),
                                                   ("yaw_180_fov_120", 180.0, -5.0, 120.0, 64)])
def test_bins_by_the_hundred_at_the_cap_and_across_atan2s_cut(gpu, exe, tmp_path, name, yaw, tilt, fov, rows):
    got = _table_case(gpu, exe, tmp_path, cc.tile("dense"), *cc.OBSERVER, yaw, cc.STEP, (rows - 1) * cc.STEP, tilt=tilt, fov=fov)
    bins = got["n_bins"]
    if name.startswith("fov_120"):
        assert 790 <= bins <= 810 and (rows * bins) % 256 != 0  # the last block of k_ceiling_cells is partly idle
    if name == "nadir":
        # The frame holds the nadir, so its border runs once around it: the bins go from one border pixel of the bottom row next to
        # the point behind the nadir to its neighbour on the other side, 11 degrees short of the whole circle (measured: 2330 bins).
        # CEIL_MAX_BINS = 2400 itself needs two border pixels within 0.45 degrees of each other as seen from the nadir, i.e. a
        # bottom row more than 127 pixels from it: no frame of 32 rows reaches the cap.
        assert 2300 < bins <= 2400 and bins * got["layout"][2] > np.radians(340.0)
    if name.startswith("yaw_180"):
        dir0, rel_lo, w = got["layout"]
        assert abs(abs(dir0) - np.pi) < 1e-12 and rel_lo < 0.0 < rel_lo + bins * w  # the bins straddle the cut at +-pi


@pytest.mark.gpu
def test_the_read_back_follows_the_frames(gpu, exe, tmp_path):
    """The second frame of a view marches with the same bytes, built once (ceiling_ms 0); a rebuilt table is the same bytes; without
    a table — ATMRT_CEILING=off, another generator, another calculator, no frame yet — the read-back reports 0 rows."""
    from atm_raytracer_amd import _abi, generators
    cfg, tiles = cc.marched("near")
    gpu.generate(_view_config(tiles, *cc.OBSERVER, 10.0, 150.0, 9_000.0), tiles)  # another view: the next frame builds its table
    gpu.generate(cfg, tiles)
    first, built = gpu.ctx.debug_ceiling_table(), gpu.work()[3]
    gpu.generate(cfg, tiles)
    second, reused = gpu.ctx.debug_ceiling_table(), gpu.work()[3]
    assert built > 0.0 and reused == 0.0, (built, reused)
    with ceiling_mode("rebuild"):
        gpu.generate(cfg, tiles)
        third, rebuilt = gpu.ctx.debug_ceiling_table(), gpu.work()[3]
    assert rebuilt > 0.0
    for t in (second, third):
        assert t["rows"] == first["rows"] == 301 and t["layout"] == first["layout"]
        assert t["cell"].tobytes() == first["cell"].tobytes() and t["suffix"].tobytes() == first["suffix"].tobytes()
    with ceiling_mode("off"):
        gpu.generate(cfg, tiles)
        off = gpu.ctx.debug_ceiling_table()
    assert off["rows"] == 0 and off["n_bins"] == 0 and off["cell"].size == 0
    gpu.generate(cfg, tiles)
    assert gpu.ctx.debug_ceiling_table()["rows"] == 301
    for generator, earth in (("Fast", None), ("Rectilinear", "FlatDistorted")):
        gpu.generate(_view_config(tiles, *cc.OBSERVER, cc.YAW, cc.STEP, cc.REACH, generator=generator, earth_shape=earth), tiles)
        assert gpu.ctx.debug_ceiling_table()["rows"] == 0, (generator, earth)
    fresh = generators.Context(0)
    try:
        assert fresh.debug_ceiling_table()["rows"] == 0
    finally:
        fresh.close()
    # capacity, then fill: a smaller capacity gets the first entries and the full size; the usual argument checks
    import ctypes as C
    lib, handle = gpu.ctx.lib, gpu.ctx.handle
    gpu.generate(cfg, tiles)
    rows, bins, lay = C.c_int32(), C.c_int32(), (C.c_double * 3)()
    cell, suffix = np.full(100, -7.0, dtype=np.float32), np.full(100, -7.0, dtype=np.float32)
    assert lib.atmrt_debug_ceiling_table(handle, 90, cell.ctypes.data, suffix.ctypes.data, C.byref(rows), C.byref(bins), lay) == 0
    assert (rows.value, bins.value, tuple(lay)) == (301, 82, first["layout"])
    assert cell[:90].tobytes() == first["cell"].ravel()[:90].tobytes() and suffix[:90].tobytes() == first["suffix"].ravel()[:90].tobytes()
    assert (cell[90:] == -7.0).all() and (suffix[90:] == -7.0).all()
    for args in ((None, 0, None, None, C.byref(rows), C.byref(bins), lay), (handle, 0, None, None, None, C.byref(bins), lay),
                 (handle, 0, None, None, C.byref(rows), None, lay), (handle, 0, None, None, C.byref(rows), C.byref(bins), None),
                 (handle, 10, None, suffix.ctypes.data, C.byref(rows), C.byref(bins), lay),
                 (handle, 10, cell.ctypes.data, None, C.byref(rows), C.byref(bins), lay)):
        assert lib.atmrt_debug_ceiling_table(*args) == _abi.ERR_INVALID_ARGUMENT, args
    # a harness call with other parameters builds another table in the buffer: the last frame's is gone, and the read-back says so
    moved = _view_config(tiles, cc.OBSERVER[0] + 0.1, cc.OBSERVER[1], cc.YAW, cc.STEP, cc.REACH)
    generators.make_generator(generators.Params(moved), gpu.terrain)._configure()
    lat, lon, dist = np.zeros(1), np.zeros(1), np.array([1000.0])
    gpu.ctx.check(lib.atmrt_coords_at_dist(handle, 46.6, 8.5, 45.0, 1, dist.ctypes.data, lat.ctypes.data, lon.ctypes.data))
    assert lib.atmrt_debug_ceiling_table(handle, 0, None, None, C.byref(rows), C.byref(bins), lay) == _abi.ERR_STATE
    gpu.generate(cfg, tiles)
    assert gpu.ctx.debug_ceiling_table()["rows"] == 301


# ---- frames marched over the spikes ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["near", "near_translucent", "far", "far_translucent", "up", "up_translucent"])
def test_frames_over_spikes_with_the_table_on_off_and_rebuilt(gpu, oracle_det, name):
    from util import assert_bitexact
    cfg, tiles = cc.marched(name)
    want = _oracle_frame(oracle_det, name)
    work = {}
    for mode in (None, "off", "rebuild"):
        with ceiling_mode(mode):
            got = gpu.generate(cfg, tiles)
            work[mode or "on"] = gpu.work()
        assert_bitexact(got, want)  # every plane, every list, n_hits and ray_steps
    on, off, rebuild = work["on"], work["off"], work["rebuild"]
    print(f"\n{name}: {int((want['hit_count'] > 0).sum())} pixels hit, {int(want['n_hits'])} trace points; lookups {on[2]} with the table, "
          f"{off[2]} without; integrated steps {on[0]} / {off[0]}; escaped rays {on[1]} / {off[1]}")
    assert on[:3] == rebuild[:3], (on, rebuild)
    assert on[2] < off[2] and on[0] <= off[0], (on, off)
    assert 0 < int((want["hit_count"] > 0).sum()) < cc.W * cc.H
    if name.startswith("up"):
        assert on[1] > 0 and on[0] < off[0], (on, off)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["yaw_180", "nadir", "two_resolutions"])
def test_frames_over_spikes_against_the_oracle(gpu, oracle_det, name):
    from util import assert_bitexact
    cfg, tiles = cc.marched(name)
    want = _oracle_frame(oracle_det, name)
    got = gpu.generate(cfg, tiles)
    on = gpu.work()
    table = gpu.ctx.debug_ceiling_table()
    with ceiling_mode("off"):
        without = gpu.generate(cfg, tiles)
        off = gpu.work()
    hit = want["hit_count"] > 0
    print(f"\n{name}: {int(hit.sum())} pixels hit, bins {table['n_bins']}; lookups {on[2]} with the table, {off[2]} without; escaped rays {on[1]}")
    assert_bitexact(got, want)
    assert_bitexact(without, want)
    assert on[2] < off[2] and 0 < hit.sum()
    if name == "nadir":  # rays between the last bin and the cut take the table's last column, the mosaic's top
        import ceiling_model
        outside = ceiling_model.bins_of(table["layout"], table["n_bins"], want["azimuth"]) == table["n_bins"]
        print(f"  {int(outside.sum())} pixels past the last of {table['n_bins']} bins, {int((outside & hit).sum())} of them hit")
        assert table["n_bins"] > 2300 and outside.sum() >= 1  # (measured: 3 pixels in the 11 degrees behind the nadir, 1 hit)
    if name == "two_resolutions":  # the rays reach the coarse tile: hits on both sides of the edge at 9 E
        lon = want["lon"][want["hit_offset"][hit].astype(np.int64)]
        assert (lon < 9.0).sum() > 50 and (lon > 9.0).sum() > 50, ((lon < 9.0).sum(), (lon > 9.0).sum())


@pytest.mark.gpu
def test_three_column_tiles_march_the_single_contexts_frame(gpu, oracle_det):
    """A tile's bins are the frame's bins: the same bits, the same integrated steps, and both the oracle's frame.  The read-back of
    the multi context is its first device's table: the same rows over the bins of that tile's columns."""
    from atm_raytracer_amd import generators
    from util import assert_bitexact, run_gpu
    import ctypes as C
    for name in ("near", "far"):
        cfg, tiles = cc.marched(name)
        single = gpu.generate(cfg, tiles)
        w_single, t_single = gpu.work(), gpu.ctx.debug_ceiling_table()
        multi = generators.Context.multi([0, 0, 0])
        try:
            tiled = run_gpu(multi, cfg, tiles)
            i, e = C.c_uint64(), C.c_uint64()
            multi.check(multi.lib.atmrt_last_march_work(multi.handle, C.byref(i), C.byref(e)))
            t_multi = multi.debug_ceiling_table()
        finally:
            multi.close()
        print(f"\n{name}: integrated steps {w_single[0]} single, {i.value} in three tiles; bins {t_single['n_bins']} / {t_multi['n_bins']} (first tile)")
        assert_bitexact(tiled, single)
        assert_bitexact(single, _oracle_frame(oracle_det, name))
        assert (int(i.value), int(e.value)) == w_single[:2]
        assert t_multi["rows"] == t_single["rows"] and 3 <= t_multi["n_bins"] < t_single["n_bins"]
        assert t_multi["layout"][0] == t_single["layout"][0] and t_multi["layout"][2] == t_single["layout"][2]
        shift = (t_multi["layout"][1] - t_single["layout"][1]) / t_single["layout"][2]  # whole bins: the tile cuts the frame's bins
        assert abs(shift - round(shift)) < 1e-6 and round(shift) >= 0


# ---- every march variant: ATMRT_MARCH_VARIANT is read once per process ----
CHILD_FRAMES = ["near", "near_translucent", "far", "up", "up_translucent", "nadir", "objects"]
CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import ceiling_cases as cc
from atm_raytracer_amd import generators
from util import frame_stats
ctx = generators.Context(0)
terrain = generators.Terrain.from_tiles(cc.tile("dense"), ctx)
resident = "dense"
out = {{}}
for name in {frames!r}:
    cfg, tiles = cc.marched(name)
    which = "sparse" if name.startswith("up") else "dense"
    if which != resident:
        ctx.check(ctx.lib.atmrt_terrain_clear(ctx.handle))
        terrain, resident = generators.Terrain.from_tiles(tiles, ctx), which
    got = generators.make_generator(generators.Params(cfg), terrain).generate()
    i, e = C.c_uint64(), C.c_uint64()
    ctx.check(ctx.lib.atmrt_last_march_work(ctx.handle, C.byref(i), C.byref(e)))
    st = frame_stats(ctx)
    out[name] = [cc.frame_hash(got), int(got["n_hits"]), int(i.value), int(e.value), int(st["terrain_lookups"]), int(st["object_rays"]), ctx.debug_march_route()]
ctx.close()
print("RESULT " + json.dumps(out))
"""
_CHILDREN = {}


def _child(variant):
    if variant not in _CHILDREN:
        env = dict(os.environ)
        for k in ("ATMRT_CEILING", "ATMRT_ESCAPE", "ATMRT_MARCH_VARIANT"):
            env.pop(k, None)
        if variant:
            env["ATMRT_MARCH_VARIANT"] = variant
        p = subprocess.run([sys.executable, "-c", CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"), frames=CHILD_FRAMES)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        _CHILDREN[variant] = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][len("RESULT "):])
    return _CHILDREN[variant]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None, "plain", "small", "sliced", "queue"])
def test_every_march_variant_marches_the_oracles_frame_over_spikes(oracle_det, variant):
    """300 steps are three slices of 128 for the sliced march: the later slices derive the ray's bin again from the pixel.  The
    frame with objects goes through the out-of-line object step of the small and the sliced march, which does not skip.  Under
    `queue` the opaque frames are marched by k_rect_march_queue, which derives every ray's bin itself (route 4); the translucent
    frames and the one with objects cannot take it and go by their size."""
    got = _child(variant)
    for name in CHILD_FRAMES:
        want = _oracle_frame(oracle_det, name)
        h, n_hits, integrated, escaped, lookups, object_rays, route = got[name]
        print(f"\n{variant or 'default'} {name}: {n_hits} trace points, integrated steps {integrated}, escaped rays {escaped}, lookups {lookups}, "
              f"object rays {object_rays}")
        assert n_hits == int(want["n_hits"]) and h == cc.frame_hash(want), (variant, name)
        if "translucent" not in name and name != "objects":  # an opaque frame's work is one number: a ray's bin is its own
            assert integrated == _child(None)[name][2], (variant, name)
        if variant == "queue":
            assert (route == 4) == ("translucent" not in name and name != "objects"), (name, route)
    tags = _oracle_frame(oracle_det, "objects")["color_tag"]
    assert (tags == 0).sum() >= 100 and (tags != 0).sum() >= 100  # terrain and objects were both met
