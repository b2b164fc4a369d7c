"""tests/interp_blend_model.py against answers computed by hand, and a census of tests/interp_blend_cases.py computed with the model
alone: the cases reach the arms, the comparisons and the sizes they claim.  No GPU.  The census asserts conditions on the INPUTS of
tests/test_gpu_interp_blend.py: if a case set fails one, the cases are wrong, not the condition."""
import itertools
import math

import numpy as np
import pytest

import interp_blend_cases as cases
import interp_blend_model as m
from interp_blend_model import Rgba, Terrain


def tp(v, distance=None, color=Terrain(1.0)):
    """A trace point whose every field is v (the distance: `distance`, if given)."""
    return m.TracePoint(v, v, v if distance is None else distance, v, v, (v, v, v), color)


# ---- hand-computed answers ----------------------------------------------------------------------------------------------------------
def test_cache_coords_floors_downwards_and_casts_like_rust():
    # -0.25 steps: floor goes down to -1, the remainder is 0.75; 2.5 steps: key 2, remainder 0.5
    points, rem_elev, rem_dir = m.cache_coords(-0.25 * 0.125, 2.5 * 0.5, 0.125, 0.5)
    assert points == [(-1, 2), (-1, 3), (0, 2), (0, 3)] and (rem_elev, rem_dir) == (0.75, 0.5)
    assert m.cache_coords(-3.0, 4.0, 1.0, 2.0) == ([(-3, 2), (-3, 3), (-2, 2), (-2, 3)], 0.0, 0.0)  # integer quotients
    assert [m.as_i32(v) for v in (2.9, -2.9, 1e300, -1e300, float("nan"), float("inf"))] == [2, -2, 2147483647, -2147483648, 0, 2147483647]


def test_trace_point_and_colour_interpolate():
    r = m.tp_interpolate(tp(1.0), tp(3.0, color=Terrain(0.5)), 0.25)  # 1 * 0.75 + 3 * 0.25; alpha 1 * 0.75 + 0.5 * 0.25
    assert r == m.TracePoint(1.5, 1.5, 1.5, 1.5, 1.5, (1.5, 1.5, 1.5), Terrain(0.875))
    assert m.color_interpolate(Terrain(0.2), Terrain(0.4), 0.5) == Terrain(0.30000000000000004)  # 0.1 + 0.2, each product exact
    assert m.color_interpolate(Rgba(0.0, 1.0, 2.0, 4.0), Rgba(4.0, 3.0, 2.0, 0.0), 0.25) == Rgba(1.0, 1.5, 2.0, 3.0)
    assert m.color_interpolate(Terrain(0.25), Rgba(1.0, 1.0, 1.0, 1.0), 0.5) == Terrain(0.25)  # the reference's mixed arms
    assert m.color_interpolate(Rgba(1.0, 1.0, 1.0, 1.0), Terrain(0.75), 0.5) == Terrain(0.75)
    assert m.same_class(Terrain(1.0), Terrain(0.0)) and not m.same_class(Terrain(1.0), Rgba(0.0, 0.0, 0.0, 1.0))


def test_two_adjacent():
    assert m.interpolate_two_adjacent(tp(2.0), tp(4.0), 0.25, 0.5).lat == 3.0
    assert m.interpolate_two_adjacent(tp(2.0), tp(4.0), cases.PRED_HALF, 0.75).lat == 3.5
    assert m.interpolate_two_adjacent(tp(2.0), tp(4.0), 0.5, 0.5) is None  # rem_elev >= 0.5


def test_two_diagonal():
    assert m.interpolate_two_diagonal(tp(2.0), tp(4.0), 0.5, 0.5).lat == 3.0     # coeff 0.25 / (0.25 + 0.25)
    assert m.interpolate_two_diagonal(tp(2.0), tp(10.0), 0.25, 0.25).lat == 2.8  # coeff 0.0625 / 0.625 = 0.1: 2 * 0.9 + 10 * 0.1 = 1.8 + 1.0
    assert m.interpolate_two_diagonal(tp(2.0), tp(4.0), 0.75, 0.25) is None and m.interpolate_two_diagonal(tp(2.0), tp(4.0), 0.25, 0.5) is None
    assert m.interpolate_two_diagonal(tp(2.0), tp(4.0), 0.5, cases.PRED_HALF) is None


def test_three():
    # rem_dir 0: interp = elem0; sum = 1 - 0.5 + 0.5 * 1 = 1; coefficient 0.5 * 1 / 1
    assert m.interpolate_three(tp(2.0), tp(100.0), tp(6.0), 0.5, 0.0).lat == 4.0
    # rem_elev 0.25, rem_dir 0.5: interp = 3; sum = 0.75 + 0.125 = 0.875; coefficient 0.125 / 0.875 = 1 / 7
    r = m.interpolate_three(tp(2.0), tp(4.0), tp(10.0), 0.25, 0.5)
    assert r.lat == 3.0 * (1.0 - 0.14285714285714285) + 10.0 * 0.14285714285714285 == 4.0
    assert m.interpolate_three(tp(2.0), tp(4.0), tp(6.0), 0.5, 0.5) is None


def test_four_and_the_angle_blend():
    assert m.interpolate_four(tp(0.0), tp(2.0), tp(4.0), tp(6.0), 0.5, 0.5).lat == 3.0
    assert m.interpolate_four(tp(0.0), tp(2.0), tp(4.0), tp(6.0), 0.25, 0.75).lat == 2.5  # 1.5 * 0.75 + 5.5 * 0.25
    pixels = [m.ResultPixel(e, a, []) for e, a in ((0.0, 8.0), (10.0, 8.0), (20.0, 8.0), (30.0, 8.0))]
    r = m.interpolate(pixels, 0.5, 0.25, 50.0)  # 0 + 10 * 0.5 * 0.25 + 20 * 0.5 * 0.75 + 30 * 0.5 * 0.25
    assert (r.elevation_angle, r.azimuth, r.trace_points) == (12.5, 8.0, [])


def test_the_match_takes_the_arm_of_the_corners_present():
    a, b, c, d = tp(1.0), tp(2.0), tp(4.0), tp(8.0)
    ix = lambda *elems: [m.Indexed(m.SEQUENCE[k], e) for k, e in elems]
    assert m.interpolate_trace_points([], 0.25, 0.25) is None
    assert m.interpolate_trace_points(ix((0, a)), 0.25, 0.25) == a and m.interpolate_trace_points(ix((0, a)), 0.5, 0.25) is None
    assert m.interpolate_trace_points(ix((1, b)), 0.25, 0.5) == b and m.interpolate_trace_points(ix((1, b)), 0.25, 0.25) is None
    assert m.interpolate_trace_points(ix((2, c)), 0.5, 0.25) == c and m.interpolate_trace_points(ix((3, d)), 0.5, 0.5) == d
    assert m.interpolate_trace_points(ix((0, a), (2, c)), 0.5, 0.25).lat == 2.5  # adjacent along elevation: (rem_dir, rem_elev) change places
    assert m.interpolate_trace_points(ix((1, b), (3, d)), 0.25, 0.75).lat == 3.5 and m.interpolate_trace_points(ix((1, b), (3, d)), 0.25, 0.5) is None
    assert m.interpolate_trace_points(ix((1, b), (2, c)), 0.5, 0.5).lat == 3.0  # diagonal with 1 - rem_dir
    assert m.interpolate_trace_points(ix((0, a), (1, b), (3, d)), 0.5, 1.0).lat == 5.0  # three(b, a, d, 0.5, 0): (2 + 8) / 2
    assert m.interpolate_trace_points(ix((0, a), (0, b)), 0.25, 0.25) == b  # match_sequence: the later point of a corner stays


def test_grouping_by_distance_and_class():
    T, R = Terrain(1.0), Rgba(0.0, 0.0, 0.0, 1.0)
    px = lambda *tps: m.ResultPixel(0.0, 0.0, list(tps))
    groups = m.collect_trace_points([px(tp(0.0, 1000.0, T), tp(1.0, 1050.0, T), tp(2.0, 1000.0, R)), px(tp(3.0, 1049.0, T), tp(4.0, 1099.0, T)),
                                     px(tp(5.0, 1120.0, T)), px()], 50.0)
    # 1050 is exactly a step from 1000: a group of its own; Rgba at 1000: another; 1049 is near 1000 (and 1050) and joins the first;
    # 1099 is a full step from 1049 but near 1050: the second group; 1120 is near 1099 only, so it joins that group through it
    assert [[(p.index, p.value.lat) for p in g] for g in groups] == \
        [[((0, 0), 0.0), ((0, 1), 3.0)], [((0, 0), 1.0), ((0, 1), 4.0), ((1, 0), 5.0)], [((0, 0), 2.0)]]
    r = m.interpolate([px(tp(0.0, 1000.0, T), tp(1.0, 1050.0, T), tp(2.0, 1000.0, R)), px(tp(3.0, 1049.0, T), tp(4.0, 1099.0, T)),
                       px(tp(5.0, 1120.0, T)), px()], 0.25, 0.0, 50.0)
    # adjacent(0, 3; rem_dir 0) = 0; three(1, 4, 5; 0.25, 0): interp = 1, sum = 0.75 + 0.25 = 1, coeff 0.25: 1 * 0.75 + 5 * 0.25, the
    # distance 1050 * 0.75 + 1120 * 0.25; the Rgba point of corner 0 alone, as it is
    assert [(t.lat, t.distance) for t in r.trace_points] == [(0.0, 1000.0), (2.0, 1067.5), (2.0, 1000.0)]
    assert [type(t.color) for t in r.trace_points] == [Terrain, Terrain, Rgba]


def test_blend_of_a_tiny_image_counts_every_referenced_point_once():
    # two pixels, keys (0, 0) and (0, 1): the lattice is their bounding rectangle, 2 x 3, and its middle column is read by both
    case = dict(name="tiny", elev=np.array([[0.5, 0.0]]) * 2.0 ** -10, dir=np.array([[0.5, 1.25]]) * 2.0 ** -9,
                min_elev_step=2.0 ** -10, min_dir_step=2.0 ** -9, simulation_step=50.0,
                lattice=dict(hit_count=np.zeros((2, 3), dtype=np.uint32), azimuth=np.array([[0.0, 2.0, 4.0], [8.0, 10.0, 12.0]]),
                             elevation_angle=np.zeros((2, 3)), px_steps=np.array([[1, 10, 100], [1000, 10000, 100000]], dtype=np.uint32),
                             lat=[], lon=[], distance=[], elevation=[], path_length=[], normal=np.zeros((0, 3)), color_tag=[], rgba=np.zeros((0, 4))))
    out = m.blend(case)
    assert out["ray_steps"] == 111111 and out["n_hits"] == 0 and out["keys"].tolist() == [[[0, 0], [0, 1]]]
    assert out["azimuth"].tolist() == [[5.0, 2.5]]  # (0 + 2 + 8 + 10) / 4; 2 * 0.75 + 4 * 0.25
    case["lattice"]["hit_count"] = np.zeros((2, 2), dtype=np.uint32)
    with pytest.raises(ValueError):
        m.blend(case)


# ---- the census -----------------------------------------------------------------------------------------------------------------------
SITES = {"single": {1: ("single.rem_elev<", "single.rem_dir<"), 2: ("single.rem_elev<", "single.rem_dir>="), 4: ("single.rem_elev>=", "single.rem_dir<"),
                    8: ("single.rem_elev>=", "single.rem_dir>=")},
         "adjacent": {k: ("adjacent.rem_elev>=",) for k in (3, 5, 10, 12)},
         "diagonal": {k: ("diagonal.rem_elev>=", "diagonal.rem_dir<", "diagonal.rem_elev<", "diagonal.rem_dir>=") for k in (9, 6)},
         "three": {k: ("three.rem_elev>=", "three.rem_dir>=") for k in (7, 11, 13, 14)}}


def census(group):
    out = m.Census()
    for case in cases.cases(group):
        c = m.expected(case)[1]
        out.groups += c.groups
        out.pixel_totals += c.pixel_totals
        out.pixel_groups += c.pixel_groups
        for k, v in c.sides.items():
            out.sides.setdefault(k, set()).update(v)
    return out


def test_census_table_reaches_every_arm_both_ways_and_every_comparison_from_three_sides():
    c = census("a")
    for mask in range(1, 16):
        assert (mask, True) in c.groups, mask
        assert mask == 15 or (mask, False) in c.groups, mask
    assert (15, False) not in c.groups
    wanted = {(arm, site) for kind in SITES.values() for arm, sites in kind.items() for site in sites}
    assert len(wanted) == 28 and set(c.sides) == wanted
    for key, sides in c.sides.items():
        assert sides == {-1, 0, 1}, (key, sides)  # met from below, at equality, from above
    # 16 masks x 6 x 6 remainders, each at least once, the remainders the blend computes being those the case names
    seen = set()
    for case in cases.cases("a"):
        rems = m.expected(case)[0]["rems"].reshape(-1, 2)
        seen |= {(case["mask"], float(e), float(d)) for e, d in rems}
    assert seen == set(itertools.product(range(16), cases.REMS6, cases.REMS6)) and len(seen) == 576
    assert cases.REMS6[2] == math.nextafter(0.5, 0.0) < 0.5 and cases.REMS6[5] == math.nextafter(1.0, 0.0) < 1.0
    assert len(cases.cases("a")) == 64 and all(max(c.pixel_groups) <= 1 for c in (m.expected(k)[1] for k in cases.cases("a")))


def test_census_grouping_scenarios_give_the_groups_they_name():
    case, = cases.cases("b")
    groups = dict(zip(case["scenario"], m.expected(case)[1].pixel_groups))
    assert groups == {"exactly-a-step-apart": 2, "an-ulp-closer": 1, "equal-distance-other-class": 2, "joins-the-first-of-two": 2,
                      "through-the-second-member": 1, "creation-order": 3, "other-class-between": 2}


def test_census_handover_holds_totals_of_four_and_five_and_every_split():
    case, = cases.cases("c")
    c = m.expected(case)[1]
    assert {0, 1, 2, 3, 4, 5} <= set(c.pixel_totals)
    count = case["lattice"]["hit_count"]
    out = m.expected(case)[0]
    splits = set()
    for p4, p5 in case["pairs"]:
        assert c.pixel_totals[p4] == 4 and c.pixel_totals[p5] == 5 and c.pixel_groups[p5] == c.pixel_groups[p4] + 1
        ke, kd = out["keys"].reshape(-1, 2)[p4] - out["keys"].reshape(-1, 2).min(axis=0)
        splits.add(tuple(int(count[ke + i, kd + j]) for i, j in m.SEQUENCE))
    assert len(case["pairs"]) == 35 and splits == {s for s in itertools.product(range(5), repeat=4) if sum(s) == 4}


def test_census_arena_holds_many_groups_and_many_arena_pixels_in_both_blocks():
    by_name = {case["name"]: case for case in cases.cases("d")}
    assert m.expected(by_name["arena-64-points"])[1].pixel_totals == [64] and 2 <= m.expected(by_name["arena-64-points"])[1].pixel_groups[0] <= 8
    c = m.expected(by_name["arena-320-groups"])[1]
    assert c.pixel_totals == [320] and c.pixel_groups == [320] and c.pixel_groups[0] > 255
    assert m.expected(by_name["arena-320-groups"])[0]["n_hits"] == 80  # the groups 240 .. 319, of the last corner
    image = by_name["arena-mixed-image"]
    totals = np.array(m.expected(image)[1].pixel_totals).reshape(3, 257)
    assert image["elev"].shape == (3, 257) and (totals > 4).sum() >= 300 and (totals <= 4).sum() >= 300
    for y in range(3):  # arena and in-register pixels in both blocks of every row, the one-lane block included
        assert (totals[y, :256] > 4).any() and (totals[y, :256] <= 4).any()
    assert (totals[:, 256] > 4).any() and (totals[:, 256] <= 4).any()


def test_census_keys_cover_both_signs_integers_and_the_last_lane():
    big = [c for c in cases.cases("e") if c["elev"].size > 1]
    assert len(big) == 2
    for k, case in enumerate(big):
        out = m.expected(case)[0]
        keys, rems = out["keys"].reshape(-1, 2), out["rems"].reshape(-1, 2)
        assert case["elev"].shape == (3, 257) and (keys < 0).any() and (keys > 0).any() and (rems == 0.0).any()
        assert ((case["elev"] < 0) & (out["rems"][..., 0] > 0)).any()  # a negative quotient that is no integer: the floor goes down
        last, rest = keys[-1], keys[:-1]
        if k == 0:
            assert last[0] < rest[:, 0].min() and last[1] > rest[:, 1].max()
        else:
            assert last[0] > rest[:, 0].max() and last[1] < rest[:, 1].min()
    single = [c for c in cases.cases("e") if c["elev"].size == 1]
    out = m.expected(single[0])[0]
    assert single[0]["elev"][0, 0] == -0.25 * single[0]["min_elev_step"] and out["keys"].tolist() == [[[-1, -1]]] and out["rems"].tolist() == [[[0.75, 0.75]]]
    assert m.expected(single[1])[0]["rems"].tolist() == [[[0.0, 0.0]]] and m.expected(single[1])[0]["keys"].tolist() == [[[-1, -2]]]


def test_census_steps_share_points_and_leave_some_out():
    for case in cases.cases("f"):
        out = m.expected(case)[0]
        keys = out["keys"].reshape(-1, 2) - out["keys"].reshape(-1, 2).min(axis=0)
        refs = np.zeros(case["lattice"]["hit_count"].shape, dtype=int)
        for ke, kd in keys:
            refs[ke:ke + 2, kd:kd + 2] += 1
        steps = case["lattice"]["px_steps"]
        assert (refs == 0).any() and (refs > 1).any() and len(set(steps.ravel().tolist())) == steps.size
        assert out["ray_steps"] == int(steps[refs > 0].astype(np.uint64).sum()) > 2 ** 32


def test_census_sweep_runs_every_seed_and_reaches_most_arms():
    sweep = cases.cases("g")
    assert [c["name"] for c in sweep] == [f"sweep-{seed}" for seed in range(20)] and cases.SWEEP_SEEDS == tuple(range(20))
    assert all(c["elev"].shape == (3, 65) for c in sweep)
    c = census("g")
    assert len({mask for mask, _ in c.groups if mask}) >= 12
    assert max(c.pixel_totals) > 4 and min(c.pixel_totals) == 0
