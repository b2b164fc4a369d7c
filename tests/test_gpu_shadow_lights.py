"""atmrt_shadow_lights* on the GPU against tests/shadow_lights_model.py (the rule of include/atmrt.h, "shadow lights", over the oracle's
world_directions, coords_at_dist, get_elev and ray stepper): the mask, every status plane, every block plane byte for byte and the
call's counts; the compacted list's and the mask's edges over hand-made planes; the shortcut off against on; the three routes; the
shadowed image drawn from one light's status plane; the refusals.  The frames and lights are tests/shadow_lights_cases.py's;
tests/test_shadow_lights_model.py asserts without a GPU what they show.  Nothing here compares the per-point rule with
atmrt_shadow_mask's fixed direction: the two rules differ by design.  Every case prints its figures before it asserts."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import shadow_cases as sc
import shadow_lights_cases as slc
import shadow_lights_model as slm
import shadow_model as sm
import shadow_sweep_cases as ssc
from atm_raytracer_amd import _abi, config, generators
from test_gpu_shadow_sweep import FILL, configure, on_and_off
from test_gpu_shadows import SHADING
from util import run_gpu

pytestmark = pytest.mark.gpu


def assert_lights(got, want, stats, tag):
    """got: a generators.ShadowLights; want: a shadow_lights_model.Result."""
    for k in ("lit_mask", "status", "block"):
        g, w = getattr(got, k), getattr(want, k)
        if g is None:
            continue
        bad = np.flatnonzero(g.ravel() != w.ravel())
        assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), \
            f"{tag} {k}: {bad.size} of {g.size} differ, first at {bad[:5]}: {g.ravel()[bad[:5]]} vs {w.ravel()[bad[:5]]}"
    assert got.stats == stats, (tag, got.stats, stats)


@pytest.fixture(scope="module")
def models(oracle_det):
    """The model's answer per case, computed once from the frame the GPU generated and shared by the tests below."""
    made, settings = {}, {}

    def get(name, cfg, tiles, res):
        if name not in made:
            frame = slc.CASES[name][0]
            if frame not in settings:
                settings[frame] = sm.Setting(oracle_det, cfg, tiles)
            dirs = slm.lights_from_angles(oracle_det, cfg.params, slc.angles(name))
            made[name] = (dirs, slm.solve(settings[frame], res, dirs, slc.REACH))
        return made[name]

    yield get
    for s in settings.values():
        s.close()


def frame_of(ctx, name):
    cfg, tiles = sc.FRAMES[slc.CASES[name][0]]()
    return cfg, tiles, run_gpu(ctx, cfg, tiles)


def full_call(ctx, dirs, res, reach=slc.REACH, lift=0.0, **kw):
    kw.setdefault("status", True)
    kw.setdefault("block", True)
    return generators.shadow_lights(ctx, dirs, reach, lift, width=res["width"], height=res["height"], **kw)


# ---- frames against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(slc.CASES))
def test_frames_equal_the_model(gpu_ctx, oracle_det, models, name):
    cfg, tiles, res = frame_of(gpu_ctx, name)
    W, H = res["width"], res["height"]
    dirs, want = models(name, cfg, tiles, res)
    # the library's host function gives the vectors the model gives
    assert generators.lights_from_angles(cfg.params, slc.angles(name), gpu_ctx.lib).tobytes() == dirs.tobytes()
    got = full_call(gpu_ctx, dirs, res)
    t = generators.shadow_timings(gpu_ctx)
    print(f"shadow lights {name}: {W}x{H} m={want.m} lights={len(dirs)} stats={got.stats} model={want.stats_on} floor={want.floor:g} "
          f"compact {t['compact_ms']:.3f} march {t['march_ms']:.3f} download {t['download_ms']:.3f} ms")
    assert want.m == 200 and got.lit_mask.shape == (H, W) and got.status.shape == got.block.shape == (3, H, W)
    assert_lights(got, want, want.stats_on, name)
    hit = W * H - got.stats["none"]
    assert got.stats["lit"] + got.stats["shadowed"] == hit * 3
    for l, (_, _, meant) in enumerate(slc.CASES[name][1]):
        lit, dark = int((got.status[l] == sm.LIT).sum()), int((got.status[l] == sm.SHADOWED).sum())
        if slc.CASES[name][0] == "sky":
            assert lit == dark == 0 and not got.lit_mask.any() and not got.status.any() and not got.block.any()
        elif meant == slc.BOTH:
            assert lit >= 0.05 * hit and dark >= 0.05 * hit
        else:
            assert (dark if meant == slc.ALL_LIT else lit) == 0
    # two calls: the same bytes; the mask alone and the status alone: the full call's
    again = full_call(gpu_ctx, dirs, res)
    assert_lights(again, got, got.stats, name + " again")
    mask_only = full_call(gpu_ctx, dirs, res, status=False, block=False)
    assert mask_only.status is None and mask_only.block is None and mask_only.lit_mask.tobytes() == got.lit_mask.tobytes() and mask_only.stats == got.stats
    status_only = full_call(gpu_ctx, dirs, res, mask=False, block=False)
    assert status_only.lit_mask is None and status_only.status.tobytes() == got.status.tobytes() and status_only.stats == got.stats


@pytest.mark.parametrize("name", [n for n in sorted(slc.CASES) if slc.CASES[n][2]])
def test_escape_shortcut_off_equals_on(gpu_ctx, models, name):
    cfg, tiles, res = frame_of(gpu_ctx, name)
    dirs, want = models(name, cfg, tiles, res)
    on, off = on_and_off(lambda: full_call(gpu_ctx, dirs, res))
    print(f"shadow lights escape {name}: on {on.stats}, off {off.stats}")
    assert_lights(on, want, want.stats_on, name + " on")
    assert_lights(off, want, want.stats_off, name + " off")
    assert off.stats["integrated_steps"] > on.stats["integrated_steps"] and on.stats["escaped_rays"] > 0 and off.stats["escaped_rays"] == 0


# ---- the planes route over hand-made points -------------------------------------------------------------------------------------
class Planes:
    """A hand-made frame (shadow_sweep_cases.planes) in device memory."""

    def __init__(self, res):
        self.shape = res["hit_count"].shape
        self.n = res["hit_count"].size
        self.count = torch.from_numpy(res["hit_count"].astype(np.int32).ravel()).cuda()
        self.lat, self.lon, self.elev = (torch.from_numpy(np.ascontiguousarray(res[k], dtype=np.float64)).cuda() for k in ("lat", "lon", "elevation"))
        assert self.lat.numel() == self.lon.numel() == self.elev.numel() == self.n

    def lights(self, ctx, dirs, reach, lift=0.0, mask=True, status=True, block=True):
        """atmrt_shadow_lights_planes_device into buffers pre-filled with FILL -> ShadowLights."""
        spec, dirs = generators.shadow_lights_spec(dirs, reach, lift)
        n_l = dirs.shape[0]
        d_mask = torch.full((self.n,), FILL, dtype=torch.int64, device="cuda") if mask else None
        d_status = torch.full((n_l, self.n), FILL, dtype=torch.uint8, device="cuda") if status else None
        d_block = torch.full((n_l, self.n), FILL, dtype=torch.int16, device="cuda") if block else None
        st = _abi.ShadowStats()
        ptr = [None if t is None else t.data_ptr() for t in (d_mask, d_status, d_block)]
        ctx.check(ctx.lib.atmrt_shadow_lights_planes_device(ctx.handle, C.byref(spec), self.n, self.count.data_ptr(), self.lat.data_ptr(),
                                                            self.lon.data_ptr(), self.elev.data_ptr(), *ptr, C.byref(st)))
        return generators.ShadowLights(None if d_mask is None else d_mask.cpu().numpy().view(np.uint64).reshape(self.shape),
                                       None if d_status is None else d_status.cpu().numpy().reshape((n_l,) + self.shape),
                                       None if d_block is None else d_block.cpu().numpy().view(np.uint16).reshape((n_l,) + self.shape),
                                       generators._shadow_stats(st), dirs)


def sphere_world(earth=slc.SMALL_SPHERE, straight=False):
    """shadow_sweep_cases.flat_world's place (the wall tile 0..1 N, 0..1 E) on a sphere: the local frame turns with the point."""
    return config.Config.from_dict({
        "view": {"position": {"latitude": 0.5, "longitude": 0.5, "altitude": {"Absolute": 100.0}},
                 "frame": {"direction": 0.0, "fov": 10.0, "tilt": 0.0, "max_distance": 10_000.0}},
        "earth_shape": earth, "straight_rays": straight, "simulation_step": 100.0,
        "output": {"width": 4, "height": 4, "generator": "Rectilinear"}})


@pytest.fixture(scope="module")
def wall_setting(oracle_det):
    cfg = sphere_world()
    st = sm.Setting(oracle_det, cfg, ssc.wall_tile())
    yield cfg, st
    st.close()


def check_planes(ctx, setting, res, dirs, tag, reach=slc.PLANES_REACH, lift=0.0):
    """The planes call, shortcut on and off, against the model: mask, planes, counts; a second call: the same bytes."""
    want = slm.solve(setting, res, dirs, reach, lift)
    dev = Planes(res)
    on, off = on_and_off(lambda: dev.lights(ctx, dirs, reach, lift))
    print(f"shadow lights {tag}: m={want.m} floor={want.floor:g} on {on.stats} off {off.stats}")
    assert_lights(on, want, want.stats_on, tag + " on")
    assert_lights(off, want, want.stats_off, tag + " off")
    assert_lights(dev.lights(ctx, dirs, reach, lift), on, on.stats, tag + " again")
    return on, want


def wall_lights(oracle, cfg):
    """Three lights seen from (0.5 N, 0.5 E): north over the wall (1.3 .. 2.6 km from the points, 19 .. 35 degrees high) at 2 and at
    25 degrees, and one to the south 1.5 degrees under the horizontal, whose ray meets the ground (0 m) 4 km out."""
    return slm.lights_from_angles(oracle, cfg.params, [(0.0, 2.0), (0.0, 25.0), (180.0, -1.5)])


@pytest.mark.parametrize("n", slc.LIST_SIZES)
def test_list_edges(gpu_ctx, oracle_det, wall_setting, n):
    """Lists of 1, 63, 64, 65 and 257 entries under three hit patterns — a list that ends one entry into a wavefront, a last wavefront
    past the list's end: every hit pixel has the model's answer for ITS point in every plane, the others 0 / NONE / 0."""
    cfg, setting = wall_setting
    configure(gpu_ctx, cfg, ssc.wall_tile())
    dirs = wall_lights(oracle_det, cfg)
    lat, lon, elev = ssc.list_points(n)
    for pattern in slc.LIST_PATTERNS:
        hit = ssc.list_hits(n, pattern)
        on, want = check_planes(gpu_ctx, setting, ssc.planes(lat, lon, elev, hit), dirs, f"list {n} {pattern}")
        assert want.m == 50 and not on.lit_mask.ravel()[~hit].any() and not on.status[:, 0, ~hit].any() and not on.block[:, 0, ~hit].any()
        if n == 257 and pattern == "all":  # the answers differ along the list and between the lights
            assert all((want.status[l] == sm.SHADOWED).any() and (want.status[l] == sm.LIT).any() for l in (0, 1))
            assert len(set(want.block.ravel().tolist())) > 8 and len(set(want.lit_mask.ravel().tolist())) > 2


@pytest.mark.parametrize("n_lights", slc.N_LIGHTS)
def test_the_masks_edges(gpu_ctx, wall_setting, n_lights):
    """1, 2, 63 and 64 lights over the 65-point list: bit 63 and the shift's edge.  The lights all differ, and every plane is compared."""
    cfg, setting = wall_setting
    configure(gpu_ctx, cfg, ssc.wall_tile())
    dirs = slc.fan_of_lights(n_lights)
    lat, lon, elev = ssc.list_points(65)
    on, want = check_planes(gpu_ctx, setting, ssc.planes(lat, lon, elev), dirs, f"{n_lights} lights")
    assert on.status.shape == (n_lights, 1, 65)
    assert not (on.lit_mask >> np.uint64(n_lights - 1) >> np.uint64(1)).any()  # no bit above the last light's
    if n_lights == 64:
        assert (on.lit_mask >> np.uint64(63)).any() and (on.status[63] == sm.LIT).any()
        assert len({int(v) for v in on.lit_mask.ravel()}) > 1
    dev = Planes(ssc.planes(lat, lon, elev))
    assert dev.lights(gpu_ctx, dirs, slc.PLANES_REACH, status=False, block=False).lit_mask.tobytes() == on.lit_mask.tobytes()
    assert dev.lights(gpu_ctx, dirs, slc.PLANES_REACH, mask=False, block=False).status.tobytes() == on.status.tobytes()


def test_a_list_that_straddles_the_terminator(gpu_ctx, oracle_det):
    """64 points 54 km apart along 46.5 N on the 3000 km sphere and the light on the eastern horizontal of their middle: its local
    elevation runs from -30 to +30 degrees within ONE wavefront; the western points are SHADOWED at their first samples, the
    eastern ones LIT."""
    cfg, tiles, _ = ssc.wide_world(earth=slc.SMALL_SPHERE)
    configure(gpu_ctx, cfg, tiles)
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        lat, lon, elev = slc.terminator_points(64)
        dirs = [slm.light_direction(oracle_det, cfg.params.earth, *slc.TERMINATOR_LIGHT_AT)]
        on, want = check_planes(gpu_ctx, setting, ssc.planes(lat, lon, elev), dirs, "terminator")
        el = want.elevation[0].ravel()
        assert el.min() < -25.0 and el.max() > 25.0 and (np.diff(el) > 0).all()
        assert (on.status[0].ravel()[el < -1.0] == sm.SHADOWED).all() and (on.status[0].ravel()[el > 20.0] == sm.LIT).all()
    finally:
        setting.close()


def test_points_decided_without_a_march_and_the_frames_seams(gpu_ctx, oracle_det):
    """SimpleSphere: the exact zenith and nadir at (0, 0) for the lights (1, 0, 0) and (-1, 0, 0) — LIT block 0 and SHADOWED block 1,
    0 steps —, a NaN latitude (LIT, 0 steps), the pole and the date line (marched like any point)."""
    cfg = sphere_world(earth="SimpleSphere")
    configure(gpu_ctx, cfg, {})
    setting = sm.Setting(oracle_det, cfg, {})
    try:
        res = ssc.planes([0.0, math.nan, 90.0, 10.0, 10.0, -90.0], [0.0, 0.0, 0.0, 180.0, -180.0, 33.0], [100.0] * 6)
        dirs = [[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.3, -0.2, 0.1]]
        on, want = check_planes(gpu_ctx, setting, res, dirs, "zenith nadir nan pole seam")
        assert on.status[:, 0, 0].tolist() == [sm.LIT, sm.SHADOWED, sm.LIT] and on.block[:, 0, 0].tolist() == [0, 1, 0]
        assert on.status[:, 0, 1].tolist() == [sm.LIT] * 3 and on.block[:, 0, 1].tolist() == [0] * 3
        assert want.elevation[0, 0, 0] == 90.0 and want.elevation[1, 0, 0] == -90.0 and np.isnan(want.elevation[:, 0, 1]).all()
        assert not want.marched[:2, 0, 0].any() and not want.marched[:, 0, 1].any() and want.marched[:, 0, 2:].all()
        # the two unmarched pairs of point 0 and the three of point 1 count no steps: a call over those two points alone
        two = ssc.planes([0.0, math.nan], [0.0, 0.0], [100.0] * 2)
        alone, _ = check_planes(gpu_ctx, setting, two, dirs[:2], "zenith nadir nan alone")
        assert alone.stats == dict(none=0, lit=3, shadowed=1, integrated_steps=0, escaped_rays=0)
    finally:
        setting.close()


# ---- the routes -----------------------------------------------------------------------------------------------------------------
def test_routes_agree(gpu_ctx, oracle_det):
    """atmrt_shadow_lights_device, and atmrt_shadow_lights_planes_device over the frame's first trace points downloaded and uploaded
    again: the bytes and counts of atmrt_shadow_lights.  Translucent terrain: the frame call reads the lists, the planes call planes."""
    cfg, tiles, res = frame_of(gpu_ctx, "alpha")
    W, H = res["width"], res["height"]
    dirs = generators.lights_from_angles(cfg.params, slc.angles("alpha"), gpu_ctx.lib)
    host = full_call(gpu_ctx, dirs, res)
    spec, keep = generators.shadow_lights_spec(dirs, slc.REACH)
    lib, st = gpu_ctx.lib, _abi.ShadowStats()
    mask = torch.full((H, W), FILL, dtype=torch.int64, device="cuda")
    status = torch.full((3, H, W), FILL, dtype=torch.uint8, device="cuda")
    block = torch.full((3, H, W), FILL, dtype=torch.int16, device="cuda")
    gpu_ctx.check(lib.atmrt_shadow_lights_device(gpu_ctx.handle, C.byref(spec), mask.data_ptr(), status.data_ptr(), block.data_ptr(), C.byref(st)))
    assert mask.cpu().numpy().tobytes() == host.lit_mask.tobytes() and status.cpu().numpy().tobytes() == host.status.tobytes()
    assert block.cpu().numpy().tobytes() == host.block.tobytes() and generators._shadow_stats(st) == host.stats
    hit = res["hit_count"] > 0
    first = res["hit_offset"][hit].astype(np.int64)
    planes = {}
    for k in ("lat", "lon", "elevation"):
        a = np.full((H, W), np.nan)
        a[hit] = res[k][first]
        planes[k] = a.ravel()
    dev = Planes(dict(hit_count=res["hit_count"], **planes))
    got = dev.lights(gpu_ctx, dirs, slc.REACH)
    print(f"shadow lights routes: {got.stats}")
    assert_lights(got, host, host.stats, "planes route")
    assert (res["hit_count"] > 1).any()  # packed lists in the frame call
    # stats are optional
    gpu_ctx.check(lib.atmrt_shadow_lights_device(gpu_ctx.handle, C.byref(spec), mask.data_ptr(), None, None, None))
    assert mask.cpu().numpy().tobytes() == host.lit_mask.tobytes()


# ---- the shadowed image ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rect_64x32", "alpha", "objects"])
def test_shadowed_image_equals_the_oracle(gpu_ctx, oracle_det, name):
    """The light is the Shading configuration's own light_dir vector, so slopes and shadows share one light: atmrt_draw_image_shadowed
    with light 0's status plane equals oracle.draw_image over the frame with the first normals of the model's SHADOWED pixels zeroed."""
    cfg, tiles, res = frame_of(gpu_ctx, name)
    W, H = res["width"], res["height"]
    az, el, _ = slc.CASES[name][1][0]
    conf = dict(SHADING, light_zenith_angle=90.0 - el, light_dir=cfg.params.frame.direction + 180.0 - az)
    coloring = generators.into_coloring(gpu_ctx.lib, cfg.params, conf)
    light = np.array(list(coloring.light_dir))
    setting = sm.Setting(oracle_det, cfg, tiles)
    try:
        want = slm.solve(setting, res, [light], slc.REACH)
    finally:
        setting.close()
    got = full_call(gpu_ctx, [light], res)
    assert_lights(got, want, want.stats_on, name + " coloring light")
    plain = generators.draw_image(gpu_ctx, coloring, W, H)
    image = generators.draw_image(gpu_ctx, coloring, W, H, shadows=got.status[0])
    expected = oracle_det.draw_image(sm.shadowed_result(res, want.status[0]), oracle_det.into_coloring(cfg.params, conf))
    differ = int((image != plain).any(axis=2).sum())
    print(f"shadow lights draw {name}: {differ} of {W * H} pixels differ from the plain image, {int((want.status[0] == sm.SHADOWED).sum())} shadowed")
    assert image.tobytes() == expected.tobytes(), np.argwhere((image != expected).any(axis=2))[:5]
    assert differ >= 1 and not (image != plain).any(axis=2)[got.status[0] != sm.SHADOWED].any()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals(gpu_ctx, oracle_det):
    cfg, tiles, res = frame_of(gpu_ctx, "fast_50x20")
    W, H = res["width"], res["height"]
    lib, h = gpu_ctx.lib, gpu_ctx.handle
    good_dirs = generators.lights_from_angles(cfg.params, [(260.0, 2.0), (100.0, 5.0)], lib)
    reference = full_call(gpu_ctx, good_dirs, res)
    mask, status, block = np.full((H, W), 9, np.uint64), np.full((2, H, W), 9, np.uint8), np.full((2, H, W), 9, np.uint16)
    d_mask = torch.zeros((H, W), dtype=torch.int64, device="cuda")
    d_status = torch.zeros((64, H, W), dtype=torch.uint8, device="cuda")
    d_f64 = torch.zeros((H, W), dtype=torch.float64, device="cuda")
    d_cnt = torch.zeros((H, W), dtype=torch.int32, device="cuda")

    def calls(handle, spec, with_outputs=True):
        p = None if spec is None else C.byref(spec)
        m, s = (mask.ctypes.data, status.ctypes.data) if with_outputs else (None, None)
        dm, ds = (d_mask.data_ptr(), d_status.data_ptr()) if with_outputs else (None, None)
        return (lib.atmrt_shadow_lights(handle, p, m, s, block.ctypes.data, None),
                lib.atmrt_shadow_lights_device(handle, p, dm, ds, None, None),
                lib.atmrt_shadow_lights_planes_device(handle, p, W * H, d_cnt.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(),
                                                      dm, ds, None, None))

    def spec_of(dirs, reach=1e4, lift=0.0, n=None):
        spec, keep = generators.shadow_lights_spec(dirs, reach, lift)
        if n is not None:
            spec.n_lights = n
        return spec, keep

    def still_works():
        again = full_call(gpu_ctx, good_dirs, res)
        assert again.lit_mask.tobytes() == reference.lit_mask.tobytes() and again.status.tobytes() == reference.status.tobytes()
        assert again.block.tobytes() == reference.block.tobytes() and again.stats == reference.stats

    inf, nan, bad = math.inf, math.nan, (_abi.ERR_INVALID_ARGUMENT,) * 3
    one = [[1.0, 0.0, 0.2]]
    refused = [("no lights", spec_of(one, n=0)), ("65 lights", spec_of(np.ones((65, 3)))),
               ("zero light", spec_of([[1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])), ("NaN light", spec_of([[nan, 0.0, 1.0]])),
               ("infinite light", spec_of([[1.0, 0.0, 1.0], [1.0, -inf, 0.0]])), ("light too long", spec_of([[1e200, 0.0, 0.0]])),
               ("light too short", spec_of([[1e-170, 0.0, 0.0]])),
               ("reach 0", spec_of(one, reach=0.0)), ("reach < 0", spec_of(one, reach=-5.0)), ("reach NaN", spec_of(one, reach=nan)),
               ("reach inf", spec_of(one, reach=inf)), ("lift < 0", spec_of(one, lift=-0.001)), ("lift NaN", spec_of(one, lift=nan)),
               ("lift inf", spec_of(one, lift=inf)), ("m = 65536", spec_of(one, reach=6_553_600.0))]
    for what, (spec, keep) in refused:
        assert calls(h, spec) == bad, what
        assert lib.atmrt_last_error(h), what
        still_works()
    null_dir, keep = spec_of(one)
    null_dir.dir = None
    assert calls(h, null_dir) == bad and calls(h, None) == bad
    good, keep = spec_of(good_dirs)
    assert calls(h, good, with_outputs=False) == bad and b"neither" in lib.atmrt_last_error(h)
    assert calls(None, good) == bad
    still_works()
    assert (mask == 9).all() and (status == 9).all() and (block == 9).all()
    assert lib.atmrt_shadow_lights_planes_device(h, C.byref(good), 0, d_cnt.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(),
                                                 d_mask.data_ptr(), None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_shadow_lights_planes_device(h, C.byref(good), W * H, None, d_f64.data_ptr(), d_f64.data_ptr(), d_f64.data_ptr(),
                                                 d_mask.data_ptr(), None, None, None) == _abi.ERR_INVALID_ARGUMENT
    still_works()
    # no parameters, then parameters and no frame
    fresh = generators.Context(gpu_ctx.device)
    try:
        assert calls(fresh.handle, good) == (_abi.ERR_STATE,) * 3 and b"atmrt_set_params" in lib.atmrt_last_error(fresh.handle)
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, fresh))._configure()
        rc = calls(fresh.handle, good)
        assert rc[:2] == (_abi.ERR_STATE,) * 2 and b"needs a frame" in lib.atmrt_last_error(fresh.handle)
        assert rc[2] == _abi.OK and not d_mask.any() and not d_status[:2].any()  # the planes call needs no frame: all NONE here
    finally:
        fresh.close()
    multi = generators.Context.multi([gpu_ctx.device, gpu_ctx.device])
    try:
        generators.make_generator(generators.Params(cfg), generators.Terrain.from_tiles(tiles, multi))._configure()
        assert lib.atmrt_shadow_lights(multi.handle, C.byref(good), mask.ctypes.data, None, None, None) == _abi.ERR_STATE
        assert b"atmrt_shadow_lights_planes_device" in lib.atmrt_last_error(multi.handle)
        assert lib.atmrt_shadow_lights_device(multi.handle, C.byref(good), d_mask.data_ptr(), None, None, None) == _abi.ERR_STATE
    finally:
        multi.close()
