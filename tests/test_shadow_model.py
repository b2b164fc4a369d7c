"""tests/shadow_model.py (the cast-shadow rule of include/atmrt.h in numpy over the oracle) on hand-made cases with known answers,
and the condition on the inputs of tests/test_gpu_shadows.py: every frame and spec it uses holds both kinds of pixel.  No GPU."""
import math

import numpy as np
import pytest

import shadow_cases as sc
import shadow_model as sm
from atm_raytracer_amd import _abi, config
from util import run_oracle


def flat_world(straight=True, step=100.0):
    """No terrain but what a test adds, a flat earth (AzimuthalEquidistant), straight rays: heights are h0 + x tan(e)."""
    return config.Config.from_dict({
        "view": {"position": {"latitude": 0.5, "longitude": 0.5, "altitude": {"Absolute": 100.0}},
                 "frame": {"direction": 0.0, "fov": 10.0, "tilt": 0.0, "max_distance": 10_000.0}},
        "earth_shape": "AzimuthalEquidistant", "straight_rays": straight, "simulation_step": step,
        "output": {"width": 4, "height": 4, "generator": "Rectilinear"}})


def one_point(lat, lon, elev):
    """A frame of one pixel whose first trace point is (lat, lon, elev)."""
    return dict(hit_count=np.ones((1, 1), np.uint32), hit_offset=np.zeros((1, 1), np.uint64), lat=np.array([lat]), lon=np.array([lon]),
                elevation=np.array([elev]), normal=np.ones((1, 3)))


def wall_tile(height=1000, row=660):
    """One 1201 x 1201 tile (0..1 N, 0..1 E) that is 0 m but for the posts of latitude row `row` (0.55 N at 660): a wall."""
    posts = np.zeros((1201, 1201), dtype=np.int16)
    posts[row, :] = height
    return {(0, 0): posts}


def test_lattice_inside_the_first_step_and_on_a_sample():
    d, m = sm.lattice(100.0, 40.0)
    assert m == 1 and d.tolist() == [0.0, 100.0]
    d, m = sm.lattice(100.0, 300.0)  # exactly on a sample: the first d_m >= reach
    assert m == 3 and d[-1] == 300.0
    d, m = sm.lattice(100.0, 300.0000001)
    assert m == 4
    d, m = sm.lattice(0.1, 1.0)  # repeated addition, not i * step: 0.1 added ten times is 0.9999999999999999 < 1
    assert m == 11 and d[10] < 1.0
    with pytest.raises(ValueError):
        sm.lattice(1.0, 65536.5)
    assert sm.lattice(1.0, 65535.0)[1] == 65535


def test_a_wall_at_a_known_distance(oracle_det):
    """The flat map (AzimuthalEquidistant) measures 100 m as 0.0009 degrees of latitude, so the wall's crest, 0.05 degrees north of
    the point, lies 5555.6 m away, between samples 55 (0.5495 N) and 56 (0.5504 N).  The posts are 1 / 1200 degree apart and the
    surface is bilinear, so the wall is a ridge that falls to 0 m one post either side of the crest: 1000 (1 - 0.0005 * 1200) =
    400 m at sample 55, 1000 (1 - 0.0004 * 1200) = 520 m at sample 56, 0 m at sample 54 and from 57 on.  A straight ray from 100 m:
    at 9 degrees it is at 100 + 5500 tan 9 = 971 m and 987 m there: LIT; at 3.2 degrees at 407.5 m (clear of 400) and then at
    100 + 5600 tan 3.2 = 413.1 m < 520: SHADOWED at 56; at 2 degrees at 292.1 m < 400: SHADOWED at 55."""
    cfg = flat_world()
    st = sm.Setting(oracle_det, cfg, wall_tile())
    try:
        res = one_point(0.5, 0.5, 100.0)
        for elevation, want in ((9.0, (sm.LIT, 0)), (3.2, (sm.SHADOWED, 56)), (2.0, (sm.SHADOWED, 55))):
            r = sm.solve(st, res, (0.0, elevation, 10_000.0, 0.0))
            assert r.m == 100 and (int(r.status[0, 0]), int(r.block[0, 0])) == want, (elevation, r.status, r.block)
        # the reach ends at the wall: m = 55 reaches sample 55 (the 2 degree ray is shadowed there), m = 54 does not
        assert sm.solve(st, res, (0.0, 2.0, 5_500.0, 0.0)).block[0, 0] == 55
        r = sm.solve(st, res, (0.0, 2.0, 5_400.0, 0.0))
        assert r.m == 54 and r.status[0, 0] == sm.LIT and r.block[0, 0] == 0 and r.stats_off["integrated_steps"] == 54
        # away from the wall, and along it: LIT
        assert sm.solve(st, res, (180.0, 2.0, 10_000.0, 0.0)).status[0, 0] == sm.LIT
        assert sm.solve(st, res, (90.0, 2.0, 10_000.0, 0.0)).status[0, 0] == sm.LIT
        # lift raises the ray: 2 degrees from 100 + 109 m is at 401.1 m at sample 55, clear of 400, and at 404.6 m < 520 at sample 56
        assert sm.solve(st, res, (0.0, 2.0, 10_000.0, 109.0)).block[0, 0] == 56
        # a pixel without a trace point: NONE
        none = dict(res, hit_count=np.zeros((1, 1), np.uint32))
        r = sm.solve(st, none, (0.0, 2.0, 10_000.0, 0.0))
        assert r.status[0, 0] == sm.NONE and r.block[0, 0] == 0 and r.stats_on == dict(none=1, lit=0, shadowed=0, integrated_steps=0, escaped_rays=0)
    finally:
        st.close()


def test_the_points_own_sample_is_not_tested(oracle_det):
    """A point on the crest a metre under the surface it stands on (999 m under 1000 m): c_0 < 0 is not looked at.  Southward at 1
    degree the first sample lies 0.0009 degrees from the crest, beyond the ridge's foot one post (0.00083 degrees) away: T = 0
    from there on and the ray, at 1000.7 m and climbing, is LIT."""
    st = sm.Setting(oracle_det, flat_world(), wall_tile())
    try:
        r = sm.solve(st, one_point(0.55, 0.5, 999.0), (180.0, 1.0, 1_000.0, 0.0))
        assert (r.status[0, 0], r.block[0, 0]) == (sm.LIT, 0)
    finally:
        st.close()


def test_the_guard_at_a_steep_negative_elevation(oracle_det):
    """No terrain at all (T = 0): from 100 m at -60 degrees, H_1 = 100 - 100 tan 60 = -73.2 < 0: SHADOWED at 1 by the height
    test.  The guard proper needs H_{i-1} < -1000 without H_i < T_i, and terrain is never below 0 m here, so it is shown on a ray
    that starts below -1000 m and climbs steeply: H_0 = -1500 stops it at i = 1 whatever H_1 is."""
    cfg = flat_world()
    st = sm.Setting(oracle_det, cfg, {})
    try:
        r = sm.solve(st, one_point(0.5, 0.5, 100.0), (0.0, -60.0, 1_000.0, 0.0))
        assert (r.status[0, 0], r.block[0, 0]) == (sm.SHADOWED, 1)
        # climbing at 89 degrees from -1500 m: H_1 = -1500 + 100 tan 89 = 4229 m > T = 0, yet H_0 < -1000: SHADOWED at 1
        r = sm.solve(st, one_point(0.5, 0.5, -1500.0), (0.0, 89.0, 1_000.0, 0.0))
        assert (r.status[0, 0], r.block[0, 0]) == (sm.SHADOWED, 1)
        # from -999 m the guard does not hold and the ray is above 0 m from the first sample on: LIT
        r = sm.solve(st, one_point(0.5, 0.5, -999.0), (0.0, 89.0, 1_000.0, 0.0))
        assert (r.status[0, 0], r.block[0, 0]) == (sm.LIT, 0)
        # a NaN never shadows
        r = sm.solve(st, one_point(0.5, 0.5, math.nan), (0.0, 10.0, 1_000.0, 0.0))
        assert (r.status[0, 0], r.block[0, 0]) == (sm.LIT, 0)
    finally:
        st.close()


def test_heights_are_the_doubles_of_ray_paths(oracle_det):
    """The stepper driven by the model returns what oracle.ray_paths returns for (h0 = H_0, [elevation], step, m)."""
    import ctypes as C
    cfg, tiles = sc.FRAMES["rect_64x32"]()
    st = sm.Setting(oracle_det, cfg, tiles)
    try:
        L = oracle_det.lib
        for straight in (False, True):
            s = sm._Stepper()
            h0, e, m = 1234.5 + 2.0, 1.7, 50
            L.oracle_stepper_init(C.byref(s), C.addressof(st.env), int(st.spherical), st.radius, h0, float(np.float64(e) * (math.pi / 180.0)), int(straight), st.step)
            mine = np.array([h0] + [L.oracle_stepper_next(C.byref(s)).h for _ in range(m)])
            _, h = oracle_det.ray_paths(cfg.params, h0, [e], st.step, m, straight=straight, atm=cfg.atmosphere)
            assert mine.tobytes() == h[0].tobytes()
    finally:
        st.close()


@pytest.fixture(scope="module")
def frames(oracle_det):
    made = {}

    def get(name):
        if name not in made:
            cfg, tiles = sc.FRAMES[name]()
            made[name] = (cfg, run_oracle(oracle_det, cfg, tiles), sm.Setting(oracle_det, cfg, tiles))
        return made[name]

    yield get
    for _, _, s in made.values():
        s.close()


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_every_gpu_case_holds_both_kinds_of_pixel(frames, name):
    frame, spec, about_shortcut = sc.CASES[name]
    cfg, res, setting = frames(frame)
    r = sm.solve(setting, res, spec)
    hit = r.stats_on["lit"] + r.stats_on["shadowed"]
    lit = r.status == sm.LIT
    early, late = int((lit & (r.esc > 0) & (r.esc < r.m)).sum()), int((lit & ((r.esc == 0) | (r.esc == r.m))).sum())
    print(f"shadow case {name}: m={r.m} hit={hit} of {r.status.size} lit={r.stats_on['lit']} shadowed={r.stats_on['shadowed']} "
          f"escape floor={r.floor:g} LIT escaping before m={early}, not={late}, steps on/off={r.stats_on['integrated_steps']}/{r.stats_off['integrated_steps']}")
    assert r.m == 200 and r.stats_on["none"] + hit == r.status.size
    assert not ((r.status == sm.SHADOWED) & (r.esc > 0)).any(), "a ray that passed the escape test was shadowed later: the certificate is broken"
    if frame == "sky":
        assert hit == 0  # no hit pixel: nothing to take a share of
        return
    if frame == "ground":
        assert hit == r.status.size
    assert r.stats_on["lit"] >= 0.05 * hit and r.stats_on["shadowed"] >= 0.05 * hit
    if about_shortcut:
        assert early >= 1 and late >= 1
        assert r.stats_on["integrated_steps"] < r.stats_off["integrated_steps"] and r.stats_on["escaped_rays"] == early
    if frame == "flat_distorted":
        assert r.floor == math.inf and r.stats_on == r.stats_off
    if frame == "objects":
        first = res["hit_offset"].ravel()[res["hit_count"].ravel() > 0].astype(np.int64)
        assert (res["color_tag"][first] == _abi.COLOR_RGBA).any() and (res["color_tag"][first] == _abi.COLOR_TERRAIN).any()
    if frame == "alpha":
        assert (res["hit_count"] > 1).any()  # packed lists: the first point is entry hit_offset[p]
    if name == "leaves_mosaic":
        px, lat, lon, _ = sm.first_points(res)
        assert (lon < 9.0).any(), "some points lie inside the mosaic, east of whose edge (9 E) the light stands"


def test_shadowed_result_zeroes_first_normals_only():
    res = dict(hit_count=np.array([[2, 0, 1]], np.uint32), hit_offset=np.array([[0, 2, 2]], np.uint64), normal=np.ones((3, 3)))
    out = sm.shadowed_result(res, np.array([[sm.SHADOWED, sm.NONE, sm.LIT]], np.uint8))
    assert out["normal"].tolist() == [[0.0] * 3, [1.0] * 3, [1.0] * 3] and res["normal"].all()
    out = sm.shadowed_result(res, np.array([[sm.LIT, sm.NONE, sm.SHADOWED]], np.uint8))
    assert out["normal"].tolist() == [[1.0] * 3, [1.0] * 3, [0.0] * 3]
