"""The conditions on the inputs of tests/test_gpu_shadow_sweep.py, by tests/shadow_model.py alone (no GPU): the sweep, the duct, the
threshold layers and the hand-made planes of tests/shadow_sweep_cases.py reach what they are built to reach.  Every test prints its
figures before it asserts; the totals below are those of this suite's own run.

Part 1, the sweep (seeds 0 .. 39; earth: the index into EARTHS; family: 0 default, 1 configuration, 2 extreme, 3 long, 4 the two
pathological splines; on-object: first trace points that lie on an object; early: LIT rays that pass the escape test before m):

    seed generator WxH earth rays stepper family step shard on-object | azimuth elevation reach lift | m floor lit shadowed none early
    0 Fast 40x23 0 refracted Linear 0 50.0 - - | 343.0 2.88 20 0 | 1 1751 916 4 0 0
    1 Rect 8x9 1 refracted Spline 1 100.0 2:10 - | 640.8 0.40 18723 0 | 188 1751 6 66 0 0
    2 Inte 34x17 2 refracted Linear 2 50.0 - 14 | 616.5 2.11 29975 2 | 600 inf 77 501 0 0
    3 Fast 26x5 3 straight Spline 3 306.6 - - | 139.7 0.29 80000 50 | 261 1751 130 0 0 130
    4 Rect 3x8 4 refracted Spline 4 100.0 - - | 612.1 82.09 40 0 | 1 51356.2 17 0 7 0
    5 Inte 9x17 5 refracted Linear 0 100.0 - 6 | 107.0 1.52 59950 0 | 600 inf 42 75 36 0
    6 Fast 17x23 6 refracted Spline 1 100.0 - - | 356.8 2.42 11160 50 | 112 inf 147 142 102 0
    7 Rect 5x17 7 straight Linear 2 50.0 - 24 | 406.9 2.01 9890 50 | 198 1751 63 2 20 12
    8 Inte 29x9 8 refracted Spline 3 39.3 - 30 | 498.0 3.96 4368 2 | 112 inf 261 0 0 0
    9 Fast 2x12 0 refracted Spline 4 50.0 18:20 - | 30.6 0.18 14255 0 | 286 inf 1 23 0 0
    10 Rect 17x4 1 refracted Linear 0 50.0 - - | 479.3 43.15 29975 2 | 600 1751 68 0 0 68
    11 Inte 20x20 2 straight Spline 1 50.0 - - | -271.7 1.08 29975 0 | 600 1751 105 135 160 51
    12 Fast 30x18 3 refracted Linear 2 50.0 - - | 391.1 1.33 24257 0 | 486 1.00001e+07 0 0 540 0
    13 Rect 13x2 4 refracted Spline 3 100.0 10:23 - | 193.7 2.94 59950 2 | 600 1.00001e+07 25 1 0 0
    14 Inte 9x9 5 refracted Spline 4 146.2 - 9 | -39.7 1.22 80000 0 | 548 inf 29 34 18 0
    15 Fast 24x13 6 straight Linear 0 50.0 - - | 746.2 -0.95 29975 0 | 600 1751 0 312 0 0
    16 Rect 7x2 7 refracted Spline 1 50.0 1:8 - | 656.8 35.48 29975 50 | 600 inf 14 0 0 0
    17 Inte 33x23 8 refracted Spline 2 100.0 - - | 453.0 1.07 40 2 | 1 inf 745 14 0 0
    18 Fast 20x22 0 refracted Spline 3 100.0 - - | -283.9 2.60 29930 50 | 300 44672.4 440 0 0 0
    19 Rect 20x6 1 straight Spline 4 100.0 - - | 698.5 3.51 9753 2 | 98 1751 120 0 0 0
    20 Inte 30x16 2 refracted Linear 0 50.0 - - | -193.5 0.88 26003 2 | 521 1751 275 82 123 0
    21 Fast 12x3 3 refracted Linear 1 50.0 - - | 522.1 -2.75 3460 50 | 70 1751 0 36 0 0
    22 Rect 31x2 4 refracted Linear 2 283.7 - 43 | -48.3 76.53 113 2 | 1 1751 62 0 0 0
    23 Inte 23x21 5 straight Spline 3 50.0 - - | 721.2 1.39 29975 2 | 600 1751 105 378 0 0
    24 Fast 18x19 6 refracted Spline 4 114.6 - 43 | 760.1 2.53 68711 50 | 600 inf 266 76 0 0
    25 Rect 3x8 7 refracted Linear 0 100.0 5:8 - | 216.0 3.06 28183 2 | 282 inf 23 1 0 0
    26 Inte 27x17 8 refracted Linear 1 100.0 - - | 427.0 2.61 5419 0 | 55 inf 187 56 216 0
    27 Fast 15x10 0 straight Spline 2 351.8 - - | 728.7 -2.80 80000 0 | 228 1751 0 150 0 0
    28 Rect 13x23 1 refracted Spline 3 326.7 3:16 - | 73.8 58.33 80000 2 | 245 42931.4 299 0 0 299
    29 Inte 40x15 2 refracted Spline 4 210.8 - - | 213.8 2.02 80000 2 | 380 inf 64 379 157 0
    30 Fast 17x17 3 refracted Linear 0 330.6 - - | 431.4 1.04 19778 2 | 60 1751 36 236 17 0
    31 Rect 37x24 4 straight Linear 1 135.2 - - | 437.0 3.81 28944 50 | 215 1751 888 0 0 888
    32 Inte 10x2 5 refracted Linear 2 100.0 - - | -347.3 2.15 59950 50 | 600 inf 20 0 0 0
    33 Fast 8x21 6 refracted Spline 3 100.0 - - | 544.3 -1.23 40 0 | 1 inf 84 20 64 0
    34 Rect 25x6 7 refracted Spline 4 100.0 - - | 642.3 65.34 59950 50 | 600 inf 92 58 0 0
    35 Inte 18x18 8 straight Linear 0 50.0 - - | -111.3 1.36 22232 50 | 445 1751 0 162 162 0
    36 Fast 39x5 0 refracted Linear 1 50.0 - - | -387.9 0.71 2456 0 | 50 1751 193 2 0 0
    37 Rect 20x15 1 refracted Spline 2 50.0 - - | 584.2 3.65 29975 0 | 600 3847.15 238 49 13 0
    38 Inte 20x13 2 refracted Spline 3 50.0 - - | 798.5 3.42 22577 0 | 452 14539.8 61 199 0 0
    39 Fast 21x4 3 straight Spline 4 100.0 - 9 | 656.1 -1.04 26883 0 | 269 1751 0 84 0 0

    totals: 40 seeds, 23 with LIT and SHADOWED, 6 with a LIT ray escaping before m, 5 with m = 1,
    5 with a negative elevation and a SHADOWED pixel, 6 shards, 8 with a first point on an object,
    18 of 18 earth x stepper combinations with a non-empty list, missing []

Part 2, 1024 ridge points of the 16,114 posts within 150 m of the wide mosaic's top (1780 m) under the duct, 150 km (m = 1500),
lift 2 m, the certificate's floor at 2240 m:

    azimuth 90, elevation 0.3:   687 LIT, 337 SHADOWED, 157 LIT escaping before m, 25 SHADOWED after rising above the top
    azimuth 270, elevation 0.15: 584 LIT, 440 SHADOWED,   0 LIT escaping before m, 22 SHADOWED after rising above the top

256 ridge points beside the threshold, azimuth 90, elevation 0.3, 100 km (certified: from = top - step = 1680, floor 1780):

    Linear, 6371 km:      174 LIT (all escaping early), 82 SHADOWED; the refused twin is certified from 2016.76
    Natural, 3000 km:     166 LIT (all escaping early), 90 SHADOWED; the refused twin is certified from 2197.95
    Derivatives, 6371 km: 174 LIT (all escaping early), 82 SHADOWED; the refused twin is certified from 2607.98

Straight rays on a sphere of 200 km, 150 km of reach, esc_ang_max = 0.7702963 rad: at 44.2 degrees 254 LIT rays are above the
floor and ascending from their first sample on and none passes the test; at 44.0 degrees all 254 pass it.

Part 3, m = 65535 (step 100 m, 0.01 degrees down, no terrain): from 1143.79 m H_65534 = 0.00592 and H_65535 = -0.01154: SHADOWED
at 65535; from 1144.0 m: LIT.  The list points under the wall: 501 LIT and 499 SHADOWED of 1000 at 2 degrees, 642 and 358 at 9
degrees, 56 distinct block values each."""
import math

import numpy as np
import pytest

import escape_cases as ec
import shadow_model as sm
import shadow_sweep_cases as ssc
from atm_raytracer_amd import _abi
from util import run_oracle


def no_shadowed_ray_escaped(r):
    assert not ((r.status == sm.SHADOWED) & (r.esc > 0)).any(), "a ray that passed the escape test was shadowed later: the certificate is broken"


def early(r):
    """LIT rays that pass the escape test before m."""
    return int(((r.status == sm.LIT) & (r.esc > 0) & (r.esc < r.m)).sum())


# ---- 1. the seeded sweep -------------------------------------------------------------------------------------------------------------
def test_the_shadow_sweep_is_not_vacuous(oracle_det):
    both = escaping = one_step = negative_shadowed = with_objects = shards = 0
    earths, combos, generators = set(), set(), set()
    for seed in ssc.SEEDS:
        c = ssc.shadow_sweep_case(seed)
        res = run_oracle(oracle_det, c["cfg"], c["tiles"])
        st = sm.Setting(oracle_det, c["cfg"], c["tiles"])
        try:
            r = sm.solve(st, res, c["spec"])
            cubic = ssc.is_cubic(st)
        finally:
            st.close()
        no_shadowed_ray_escaped(r)
        lit, sh = r.stats_on["lit"], r.stats_on["shadowed"]
        first = res["hit_offset"].ravel()[res["hit_count"].ravel() > 0].astype(np.int64)
        on_object = int((res["color_tag"][first] == _abi.COLOR_RGBA).sum())
        if seed == ssc.SEEDS[0]:
            print("\nshadow sweep: seed generator WxH earth rays stepper family step shard on-object | azimuth elevation reach lift | m floor lit shadowed none early")
        shard = "-" if c["shard"] is None else "%d:%d" % c["shard"]
        print(f"shadow sweep: {seed} {c['generator'][:4]} {res['width']}x{res['height']} {c['earth']} {'straight' if c['straight'] else 'refracted'} "
              f"{'Spline' if cubic else 'Linear'} {c['family']} {c['step']:.1f} {shard} {on_object if c['objects'] else '-'} | "
              f"{c['spec'][0]:.1f} {c['spec'][1]:.2f} {c['spec'][2]:.0f} {c['spec'][3]:.0f} | {r.m} {r.floor:.6g} {lit} {sh} {r.stats_on['none']} {early(r)}")
        assert res["hit_count"].shape == r.status.shape and r.m <= ssc.MAX_STEPS
        both += lit > 0 and sh > 0
        escaping += early(r) > 0
        one_step += r.m == 1
        negative_shadowed += c["spec"][1] < 0.0 and sh > 0
        with_objects += on_object > 0
        shards += c["shard"] is not None
        generators.add(c["generator"])
        if lit + sh:
            earths.add(c["earth"])
            combos.add((c["earth"], cubic))
    n = len(ssc.SEEDS)
    missing = sorted(set((e, k) for e in range(9) for k in (False, True)) - combos)
    print(f"shadow sweep totals: {n} seeds, {both} with LIT and SHADOWED, {escaping} with a LIT ray escaping before m, {one_step} with m = 1, "
          f"{negative_shadowed} with a negative elevation and a SHADOWED pixel, {shards} shards, {with_objects} with a first point on an object, "
          f"{len(combos)} of 18 earth x stepper combinations with a non-empty list, missing {missing}")
    assert both >= 0.4 * n and escaping >= 0.15 * n
    assert len(generators) == 3
    if n >= 40 and ssc.SEED_FIRST == 0:
        assert one_step >= 3 and negative_shadowed >= 3
        assert earths == set(range(9))
        assert not missing, missing
        assert shards >= 1 and with_objects >= 1


# ---- 2. ducts, threshold layers and a small sphere over ridge points -------------------------------------------------------------------
def test_ridge_points_are_posts(oracle_det):
    lat, lon, elev = ssc.ridge_posts()
    tiles, top = ec.frame_tiles(wide=True)
    print(f"shadow ridge: {lat.size} posts within 150 m of the top {top:g}")
    assert lat.size >= 4096 and elev.min() > top - 151.0 and elev.max() == top - 1.0
    res = ssc.ridge_points(1024)
    t = oracle_det.terrain_new(tiles)
    try:
        # lat0 + row / (n - 1) is the post up to a rounding of the quotient: the bilinear surface there is the post's value up to 1e-9 m
        # (a post on the mosaic's north or east edge, 49 N or 11 E, belongs to a tile that is not there: no value)
        got = [(oracle_det.get_elev(t, la, lo), el, la, lo) for la, lo, el in zip(res["lat"], res["lon"], res["elevation"])]
        outside = [(la, lo) for g, _, la, lo in got if g is None]
        worst = max(abs(g - el) for g, el, _, _ in got if g is not None)
        print(f"shadow ridge: get_elev differs from the post's value by at most {worst:g} m; {len(outside)} of 1024 on the outer edge: {outside[:4]}")
        assert worst < 1.0e-6 and len(outside) <= 8 and all(la == 49.0 or lo == 11.0 for la, lo in outside)
    finally:
        oracle_det.terrain_free(t)
    assert len(set(zip(res["lat"].tolist(), res["lon"].tolist()))) >= 1000  # a post on a shared tile edge may be drawn twice


@pytest.mark.parametrize("name", sorted(ssc.DUCT_SPECS))
def test_the_duct_returns_shadow_rays_to_the_terrain(oracle_det, oracle_libm, name):
    """The floor of the certificate lies above the layer; below it, rays that rise above the mosaic's top come down again and are
    blocked: a floor at the top would have called them LIT."""
    cfg, tiles, top = ssc.duct_world()
    g = ec.G(oracle_libm, cfg.atmosphere, 6_371_000.0, cfg.params.wavelength)
    assert max(g(float(h)) for h in np.linspace(top + 61.0, top + 359.0, 50)) > 1.5
    res, spec = ssc.ridge_points(1024), ssc.DUCT_SPECS[name]
    st = sm.Setting(oracle_det, cfg, tiles)
    try:
        r = sm.solve(st, res, spec)
        back = ssc.rose_above(st, res, spec, r, top)
    finally:
        st.close()
    print(f"shadow duct {name}: m={r.m} floor={r.floor:g} lit={r.stats_on['lit']} shadowed={r.stats_on['shadowed']} early={early(r)} "
          f"SHADOWED after rising above the top={back}")
    no_shadowed_ray_escaped(r)
    assert r.m == 1500 and r.floor > top + 360.0
    assert back >= 10
    if name == "east":
        assert early(r) >= 50


def test_threshold_layers_lie_either_side_of_the_certificate(oracle_det):
    lib = ec.load_lib()
    res = ssc.ridge_points(256)
    for name, (cfg, tiles, top, certified) in sorted(ssc.threshold_worlds().items()):
        st = sm.Setting(oracle_det, cfg, tiles)
        try:
            _, start, _ = ec.certificate(lib, cfg.atmosphere, st.radius, cfg.params.wavelength, top, st.step)
            r = sm.solve(st, res, ssc.THRESHOLD_SPEC)
        finally:
            st.close()
        print(f"shadow threshold {name}: from={start:g} floor={r.floor:g} m={r.m} lit={r.stats_on['lit']} shadowed={r.stats_on['shadowed']} early={early(r)}")
        no_shadowed_ray_escaped(r)
        assert (start == top - st.step) == certified, (name, start)
        assert r.m == 1000 and r.stats_on["lit"] > 0
        if certified:
            assert r.floor == top and early(r) > 0
        else:
            assert r.floor > top


def test_the_angle_bound_bites_on_a_small_sphere(oracle_det):
    cfg, tiles, top = ssc.straight_sphere_world()
    res = ssc.ridge_points(256)
    st = sm.Setting(oracle_det, cfg, tiles)
    try:
        for name, spec in sorted(ssc.STRAIGHT_SPHERE_SPECS.items()):
            r = sm.solve(st, res, spec)
            floor, ang_max = st.escape(spec[2])
            ang = spec[1] * (math.pi / 180.0)
            refused = 0  # LIT rays that are above the floor and ascending at some sample and yet never pass the test
            for p, el in zip(*sm.first_points(res)[::3]):
                if r.status.ravel()[p] == sm.LIT and r.esc.ravel()[p] == 0:
                    H, up = ssc.ray_heights(st, float(el + spec[3]), spec[1], 3)
                    refused += bool(np.any((H[1:] > floor) & up[1:]))
            print(f"shadow small sphere {name}: esc_ang_max={ang_max:.7f} angle={ang:.7f} floor={floor:g} m={r.m} lit={r.stats_on['lit']} "
                  f"shadowed={r.stats_on['shadowed']} early={early(r)} refused by the angle={refused}")
            no_shadowed_ray_escaped(r)
            assert r.m == 1500 and floor == top and abs(ang_max - 0.7702963) < 1e-6
            if name == "bites":
                assert not ang < ang_max and refused >= 100 and early(r) == 0 and r.stats_on == r.stats_off
            else:
                assert ang < ang_max and refused == 0 and early(r) >= 100
    finally:
        st.close()


# ---- 3. known answers, list edges, range ends ----------------------------------------------------------------------------------------
def test_known_answers_as_planes(oracle_det):
    """The table of shadow_sweep_cases.KNOWN holds the answers tests/test_shadow_model.py derives by hand, and the model gives them
    over one-pixel planes; the point with a NaN latitude: every geodesic point is NaN, T is 0 or NaN, H < T false: LIT."""
    cfg = ssc.flat_world()
    settings = {True: sm.Setting(oracle_det, cfg, ssc.wall_tile()), False: sm.Setting(oracle_det, cfg, {})}
    try:
        for name, wall, point, spec, want in ssc.KNOWN:
            r = sm.solve(settings[wall], ssc.planes(*point), spec)
            assert (int(r.status[0, 0]), int(r.block[0, 0])) == want, name
    finally:
        for s in settings.values():
            s.close()


def test_list_points_differ_along_the_row(oracle_det):
    """Under the 2 degree light the block index falls along the row (a permuted list would show) and the last points, beyond the
    wall, are LIT; under 9 degrees the points next to the wall are SHADOWED and the rest LIT."""
    st = sm.Setting(oracle_det, ssc.flat_world(), ssc.wall_tile())
    try:
        for name, spec in sorted(ssc.LIST_SPECS.items()):
            r = sm.solve(st, ssc.planes(*ssc.list_points(1000)), spec)
            blocks = r.block.ravel()
            print(f"shadow list {name}: lit={r.stats_on['lit']} shadowed={r.stats_on['shadowed']} distinct blocks={np.unique(blocks).size} "
                  f"first 65: lit={int((r.status.ravel()[:65] == sm.LIT).sum())} last 65: lit={int((r.status.ravel()[-65:] == sm.LIT).sum())}")
            assert r.stats_on["lit"] >= 50 and r.stats_on["shadowed"] >= 50
            assert np.unique(blocks).size >= (40 if name == "2deg" else 5)
            assert np.unique(blocks[:63]).size >= 2  # the shortest lists hold different answers too
    finally:
        st.close()


def test_the_last_sample_of_the_longest_ray(oracle_det):
    """m = 65535: from FAR_BLOCKED the ray is below 0 m first at its last sample, from FAR_LIT never."""
    st = sm.Setting(oracle_det, ssc.flat_world(), {})
    try:
        r = sm.solve(st, ssc.planes([0.5, 0.5], 0.5, [ssc.FAR_BLOCKED, ssc.FAR_LIT]), ssc.FAR_SPEC)
        H, _ = ssc.ray_heights(st, ssc.FAR_BLOCKED, ssc.FAR_SPEC[1], 65535)
        print(f"shadow far: m={r.m} status={r.status.ravel()} block={r.block.ravel()} heights {ssc.FAR_BLOCKED} and {ssc.FAR_LIT}: "
              f"H_65534={H[65534]:.5f} H_65535={H[65535]:.5f}")
        assert r.m == 65535 and r.status.ravel().tolist() == [sm.SHADOWED, sm.LIT] and r.block.ravel().tolist() == [65535, 0]
        assert r.stats_off["integrated_steps"] == 2 * 65535 == r.stats_on["integrated_steps"]
    finally:
        st.close()
