"""The rule of include/atmrt.h, "apparent elevation", by its model alone (tests/sky_apparent_model.py), without a GPU: the tail
rule and every arm of the inverse against answers computed by hand on hand-made tables; the closure of the inverse against the
exact route (tests/sky_model.py's ray) over the lattice the feature was proposed with; and the sunset case, which tells the
true-direction shadow lights from the geometric ones.  Every figure is printed before it is asserted.

Measured (US-76, sky step 1000 m, top 100 km, de = 0.02 degrees, rows 281.25 m apart; DESIGN.md §7 item 15 records it): on the
sphere of 6371 km the worst closure is 1.07e-4 degrees (9.0e-5, 1.07e-4 and 1.01e-4 for the pairs at 0, 4000 and 8000 m), under the
bound of 2e-4; on a flat earth 1.10e-2 degrees next to the lowest exiting ray, where no bound is asserted."""
import math
import struct

import numpy as np

import shadow_lights_model as slm
import shadow_model as sm
import shadow_sweep_cases as ssc
import sky_apparent_cases as sac
import sky_apparent_model as sam
import sky_model as skm


def same(a, b):
    return struct.pack("d", a) == struct.pack("d", b) or (math.isnan(a) and math.isnan(b))


# ---- answers computed by hand ----------------------------------------------------------------------------------------------------
def test_the_tail_rule_by_hand():
    seen = set()
    for T, S, want in sac.TAIL_ROWS:
        got = sam.tail_of(T, S)
        assert got == want, (T, S, got, want)
        seen.add(got)
    n_el = sac.HAND_EL[2]
    assert {0, n_el - 2, n_el - 1, n_el} <= seen
    assert sam.usable([t for _, _, t in sac.TAIL_ROWS], n_el).tolist() == [True, True, True, True, True, False, False, False, False]
    assert sam.tails(np.array(sac.HAND_T), np.array(sac.HAND_S)).tolist() == sac.HAND_TAIL


def test_every_arm_of_the_row_inverse_by_hand():
    table = sac.hand_table()
    assert table.tail.tolist() == sac.HAND_TAIL and table.usable.all()
    arms = set()
    for j, t, want, arm in sac.ROW_ANSWERS:
        got, got_arm = sam.row(table.spec, table.T[j], int(table.tail[j]), t)
        assert same(got, want) and got_arm == arm, (j, t, got, want, got_arm, arm)
        arms.add((j, arm))
    assert {(j, a) for j in range(3) for a in ("inside", "below", "above")} <= arms and (0, "nan") in arms
    T, _, tail = sac.TAIL_ROWS[3]
    assert tail == table.spec.n_el - 2
    for t, want, arm in sac.LAST_TAIL_ANSWERS:
        got, got_arm = sam.row(table.spec, T, tail, t)
        assert same(got, want) and got_arm == arm, (t, got, want, got_arm, arm)


def test_apparent_by_hand():
    table = sac.hand_table()
    for h, t, want in sac.APPARENT_ANSWERS:
        got = sam.apparent(table, h, t)
        assert same(got, want), (h, t, got, want)
        assert same(sam.apparent(table, h, t, straight=True), t)  # straight rays: t itself, no table consulted
    js = {sam.apparent_parts(table, h, t)[1:3] for h, t, _ in sac.APPARENT_ANSWERS}
    assert {(0, 0.0), (1, 0.0), (1, 1.0), (0, 0.5), (1, 0.5), (None, None)} <= js


def test_spec_limits():
    good = dict(alt=(0.0, 9000.0, 33), el=(-4.0, 88.0, 4601))
    assert sam.Spec(**good).valid()
    nan, inf = math.nan, math.inf
    for alt, el, kw in [((0.0, 0.0, 3), good["el"], {}), ((5.0, 0.0, 3), good["el"], {}), ((nan, 1.0, 3), good["el"], {}), ((0.0, inf, 3), good["el"], {}),
                        (good["alt"], (-90.0, 10.0, 5), {}), (good["alt"], (-4.0, 90.0, 5), {}), (good["alt"], (3.0, 3.0, 5), {}),
                        (good["alt"], (5.0, 3.0, 5), {}), (good["alt"], (nan, 3.0, 5), {}), ((0.0, 1.0, 1), good["el"], {}),
                        ((0.0, 1.0, 1025), good["el"], {}), (good["alt"], (-4.0, 8.0, 1), {}), (good["alt"], (-4.0, 8.0, 65537), {}),
                        ((0.0, 1.0, 257), (-4.0, 8.0, 65536), {}), (good["alt"], good["el"], dict(step=0.0)), (good["alt"], good["el"], dict(top=-1.0)),
                        (good["alt"], good["el"], dict(m=0))]:
        assert not sam.Spec(alt, el, **kw).valid(), (alt, el, kw)
    assert sam.Spec((0.0, 1.0, 256), (-4.0, 8.0, 65536)).valid() and sam.Spec((0.0, 1.0, 1024), (-4.0, 8.0, 16384)).valid()


# ---- the closure against the exact route -----------------------------------------------------------------------------------------
def closure(setting, alt_lo):
    """-> (the largest |true elevation marched back - target| [deg], where, how many marches, the tail start) for one row pair."""
    table = sam.build(setting, sac.closure_spec(alt_lo))
    assert table.usable.all(), table.tail
    start, targets = sac.closure_targets(table)
    assert len(targets) >= 100 and (targets <= start + 1.0).sum() >= len(targets) // 2 and targets.max() <= sac.CLOSURE_TOP_TARGET
    worst, where, n = 0.0, None, 0
    s = table.spec
    for f in (0.0, 0.5, 1.0):
        h = s.alt_lo + f * s.dh
        for t in targets:
            e = sam.apparent(table, h, t)
            status, _, true = skm.ray(setting, h, e, s.step, s.top, s.floor, s.m)
            assert status == skm.EXIT, (alt_lo, f, t, e, status)
            n += 1
            if abs(true - t) > worst:
                worst, where = abs(true - t), (f, float(t), e)
    return worst, where, n, start


def test_closure_on_the_sphere(oracle_det):
    """Every inverted elevation, marched from h by the exact route, EXITs within 2e-4 degrees of its target."""
    setting = skm.Setting.of_config(oracle_det, sac.setting_cfg())
    worst = 0.0
    for alt_lo in sac.CLOSURE_ROWS:
        w, where, n, start = closure(setting, alt_lo)
        print(f"apparent closure sphere rows {alt_lo:g} / {alt_lo + sac.CLOSURE_DH:g} m: {n} marches from true {start:.4f} deg, worst {w:.3e} deg at (f, t, e) = {where}")
        worst = max(worst, w)
    print(f"apparent closure sphere: worst {worst:.3e} deg, bound {sac.CLOSURE_BOUND:.1e}")
    assert worst <= sac.CLOSURE_BOUND


def test_closure_on_a_flat_earth_is_measured_only(oracle_det):
    """Next to the lowest exiting ray of a flat refracting earth the true elevation bends sharply against the launch elevation: the
    figure is printed and recorded, no bound is asserted."""
    setting = skm.Setting.of_config(oracle_det, sac.setting_cfg(earth="FlatDistorted"))
    w, where, n, start = closure(setting, 0.0)
    print(f"apparent closure flat rows 0 / {sac.CLOSURE_DH:g} m: {n} marches from true {start:.4f} deg, worst {w:.3e} deg at (f, t, e) = {where}")
    assert math.isfinite(w)


# ---- the sunset ------------------------------------------------------------------------------------------------------------------
def test_the_sunset_tells_the_two_rules_apart(oracle_det):
    """Sea-level points 2 m up on the 6371 km sphere, no terrain, a light at the local true elevation -0.3 degrees, reach 5 km: the
    geometric rule launches every ray 0.3 degrees down and shadows every point; under the true-direction rule the light appears
    about 0.2 degrees up and every point is LIT."""
    cfg = sac.sunset_cfg()
    setting = sm.Setting(oracle_det, cfg, {})
    try:
        table = sam.build(skm.Setting.of_config(oracle_det, cfg), sac.table_spec())
        assert table.usable.all()
        lat, lon, elev = sac.sunset_points()
        res = ssc.planes(lat, lon, elev)
        dirs = [slm.light_direction(oracle_det, cfg.params.earth, *sac.SUNSET_AT, 90.0, sac.SUNSET_TRUE_ELEVATION)]
        geometric = slm.solve(setting, res, dirs, sac.SUNSET_REACH, sac.SUNSET_LIFT)
        true = sam.solve_true(setting, table, res, dirs, sac.SUNSET_REACH, sac.SUNSET_LIFT)
        el = true.elevation[0].ravel()
        print(f"sunset: true {true.true_elevation.min():.5f} .. {true.true_elevation.max():.5f} deg, apparent {el.min():.5f} .. {el.max():.5f} deg; "
              f"geometric {geometric.stats_on}, true {true.stats_on}")
        assert np.abs(true.true_elevation - sac.SUNSET_TRUE_ELEVATION).max() < 1e-3
        assert (geometric.status == sm.SHADOWED).all() and not geometric.lit_mask.any()
        assert (true.status == sm.LIT).all() and (true.lit_mask == 1).all()
        assert (el > 0.1).all() and (el < 0.3).all()
    finally:
        setting.close()


def test_the_library_tables_reach_what_they_are_built_for(oracle_det):
    """The settings of the GPU tests, by the model: their statuses, usable or not, and a census of the arms the pair list reaches."""
    tables = {}
    for name in sac.SETTINGS:
        cfg, top = sac.setting_of(name)
        table = tables[name] = sam.build(skm.Setting.of_config(oracle_det, cfg), sac.table_spec(3, 257, top))
        kinds = sorted(set(table.S.ravel().tolist()))
        print(f"apparent table {name}: statuses {kinds}, tail {table.tail.tolist()}")
        if name == "spline100":
            assert (table.tail == 257).all() and skm.EXIT not in kinds and skm.LOST in kinds
        else:
            assert table.usable.all() and skm.GROUND in kinds and skm.EXIT in kinds
        if name == "straight":
            exits = table.S == skm.EXIT
            assert all(same(table.T[j, k], table.spec.el(k)) for j, k in zip(*np.nonzero(exits)))
    table = tables["us76_sphere"]
    h, t = sac.census_pairs(table)
    parts = [sam.apparent_parts(table, a, b) for a, b in zip(h, t)]
    arms = {p[3] for p in parts} | {p[4] for p in parts}
    assert {"inside", "below", "above", "nan", None} <= arms
    assert any(a < table.spec.alt_lo for a in h) and any(a > table.spec.alt_hi for a in h)
