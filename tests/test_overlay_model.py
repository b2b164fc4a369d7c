"""Known answers of tests/overlay_model.py, the numpy restatement of renderer::output_image's annotations (src/renderer/mod.rs:28-365)
that the overlay entry points of the library are checked against.  No library, no GPU."""
import numpy as np

import overlay_model as om


def test_num_decimals_known_answers():
    """The cases of the reference's only unit test (renderer/mod.rs:445-458)."""
    cases = {0.0: 0, 1.0: 0, 15.0: 0, 183.0: 0, 0.1: 1, 0.3: 1, 0.9: 1, 1.8: 1, 12.6: 1, 133.5: 1, 0.25: 2, 33.99: 2, 33.01: 2,
             133.01002: 5}
    assert len(cases) == 14
    for x, want in cases.items():
        assert om.num_decimals(x) == want, x
    assert om.rust_round(0.5) == 1.0 and om.rust_round(-2.5) == -3.0 and om.rust_round(2.4999) == 2.0  # half away from zero
    assert om.num_decimals(1.0 / 3.0) == 10  # no power of ten below 10^10 brings it within 0.001 of an integer: the fall-back
    assert om.fmt(-0.04, 1) == "-0.0" and om.fmt(359.96, 1) == "360.0" and om.fmt(0.125, 2) == "0.12" and om.fmt(45.0, 0) == "45"


def pixels(points):
    return sorted(points)


def test_bresenham_hand_drawn_segments():
    seg = om.segment_pixels
    assert seg(3, 5, 4, 5) == [(3, 5), (4, 5)]                                   # dy = 0
    assert seg(3, 5, 4, 6) == [(3, 5), (4, 6)] and seg(3, 5, 4, 4) == [(3, 5), (4, 4)]  # dy = +-1: the two end points
    # dy = +-2: steep, running over y; error = 1 -> 0 after the first pixel (no step), -1 after the second (step)
    assert seg(3, 5, 4, 7) == [(3, 5), (3, 6), (4, 7)]
    assert seg(3, 5, 4, 3) == [(4, 3), (4, 4), (3, 5)]  # ordered so that y ascends: starts at the far end
    assert pixels(seg(4, 3, 3, 5)) == pixels(seg(3, 5, 4, 3))                     # both directions, same pixels
    # dy = +-5: error 2.5 -> 1.5, 0.5, -0.5 after the first, second and third pixel: the step falls after the third
    assert seg(0, 0, 1, 5) == [(0, 0), (0, 1), (0, 2), (1, 3), (1, 4), (1, 5)]
    assert seg(0, 5, 1, 0) == [(1, 0), (1, 1), (1, 2), (0, 3), (0, 4), (0, 5)]
    assert pixels(seg(1, 0, 0, 5)) == pixels(seg(0, 5, 1, 0))
    # end points are always drawn
    for x0, y0, x1, y1 in [(2, 9, 3, 0), (2, 0, 3, 9), (0, 0, 7, 3), (7, 3, 0, 0)]:
        p = seg(x0, y0, x1, y1)
        assert (x0, y0) in p and (x1, y1) in p and len(p) == max(abs(x1 - x0), abs(y1 - y0)) + 1
    # clipped: pixels outside the image are skipped, not moved to the border
    img = np.zeros((4, 4, 3), dtype=np.uint8)
    om.draw_line_segment(img, (2, 0), (2, 9), (255, 255, 255))
    assert img[:, 2].all() and img.sum() == 4 * 3 * 255
    img[:] = 0
    om.draw_line_segment(img, (0, 6), (3, 6), (1, 2, 3))
    assert img.sum() == 0


def test_find_elev_on_hand_made_planes():
    col = lambda values: np.array(values, dtype=np.float64).reshape(-1, 1)
    # a tie takes the first row: rows 1 and 2 are both 0.5 away from 0
    assert om.find_elev(col([2.0, 0.5, -0.5, -1.5]), 0, 0.0) == 1
    # a NaN row is skipped and never wins
    assert om.find_elev(col([2.0, np.nan, 1.0, 0.2, -1.0]), 0, 0.0) == 3
    assert om.find_elev(col([2.0, np.nan, 0.2, -1.0]), 0, 0.0) is None  # ... but as the NEIGHBOUR of the best row it fails the test
    assert om.find_elev(col([np.nan, np.nan, np.nan]), 0, 0.0) is None
    # a target off the plane: the closest row is the edge, further away than 1.5 rows
    assert om.find_elev(col([3.0, 2.0, 1.0]), 0, -1.0) is None
    assert om.find_elev(col([3.0, 2.0, 1.0]), 0, -0.4) == 2  # 1.4 rows beyond the edge still counts
    # best = 0 takes row 1 as its neighbour
    assert om.find_elev(col([3.0, 2.0, 1.0]), 0, 4.4) == 0 and om.find_elev(col([3.0, 2.0, 1.0]), 0, 4.6) is None
    plane = np.hstack([col([2.0, 0.5, -0.5, -1.5, -2.5]), col([2.0, np.nan, 1.0, 0.2, -1.0]), col([13.0, 12.0, 11.0, 10.0, 9.0])])
    assert om.find_elev_all(plane, 0.0) == [1, 3, None] == [om.find_elev(plane, x, 0.0) for x in range(3)]
    rng = np.random.default_rng(5)
    plane = np.cumsum(-rng.uniform(0.0, 0.2, size=(40, 17)), axis=0) + rng.uniform(1.0, 5.0, size=17)
    plane[rng.integers(0, 40, 12), rng.integers(0, 17, 12)] = np.nan
    for target in (0.0, -2.5, 9.0):
        assert om.find_elev_all(plane, target) == [om.find_elev(plane, x, target) for x in range(17)]


def fast_frame(direction, fov, w, h, tilt=0.0):
    """Azimuth row / elevation column of a Fast-style frame: linear in the pixel index, azimuth wrapped once into [0, 360)."""
    az = direction + (np.arange(w) - w / 2.0) * fov / w
    az = np.where(az < 0.0, az + 360.0, np.where(az >= 360.0, az - 360.0, az))
    el = tilt - (np.arange(h) - h / 2.0) * fov / w
    return np.tile(az, (h, 1)), np.tile(el.reshape(-1, 1), (1, w))


def test_tick_resolution_on_an_analytic_fast_row():
    w, h = 200, 100
    frame = {"direction": 40.0, "fov": 20.0, "width": w, "height": h, "tilt": 0.0}
    az, el = fast_frame(40.0, 20.0, w, h)
    # Single: azimuth 45 is column 150 exactly
    hor, ver = om.gen_ticks(frame, [("Single", 45.0, 15, True)], [], az, el)
    assert hor == {150: {"size": 15, "labelled": True, "label": "45"}} and ver == {}
    assert om.gen_ticks(frame, [("Single", 75.0, 15, True)], [], az, el)[0] == {}  # outside the frame
    # Multiple with bias: 31.5, 36.5, 41.5, 46.5; decimals come from the STEP of a labelled Multiple (5 -> 0) and the angle of a
    # labelled Single (0.25 -> 2)
    hor, _ = om.gen_ticks(frame, [("Multiple", 1.5, 5.0, 7, True), ("Single", 33.25, 3, True)], [], az, el)
    assert {x: t["label"] for x, t in hor.items()} == {15: "31.50", 65: "36.50", 115: "41.50", 165: "46.50", 32: "33.25"}
    hor, _ = om.gen_ticks(frame, [("Multiple", 1.5, 5.0, 7, True), ("Single", 33.25, 3, False)], [], az, el)
    assert hor[15]["label"] == "32" and hor[32] == {"size": 3, "labelled": False, "label": "33"}  # an unlabelled tick adds no decimals
    # a collision of two definitions: the larger size stays; the earlier one on equal size
    hor, _ = om.gen_ticks(frame, [("Multiple", 0.0, 2.0, 5, False), ("Multiple", 0.0, 10.0, 10, True), ("Single", 40.0, 10, False)], [], az, el)
    assert hor[100] == {"size": 10, "labelled": True, "label": "40"} and hor[120]["size"] == 5 and len(hor) == 10
    # a wrap through 360: direction 355, the row runs 345 .. 359.9, 0 .. 4.9; current_az 360 is labelled 0 and found through
    # diff_azimuth's single wrap
    frame = {"direction": 355.0, "fov": 20.0, "width": w, "height": h, "tilt": 0.0}
    az, el = fast_frame(355.0, 20.0, w, h)
    hor, _ = om.gen_ticks(frame, [("Multiple", 0.0, 5.0, 4, True)], [], az, el)
    assert {x: t["label"] for x, t in hor.items()} == {0: "345", 50: "350", 100: "355", 150: "0"}
    # vertical: elevation runs from +5 at the top down to -4.9; Multiple every 2.5 degrees starts AT min_elev = -5 (ceil of a whole
    # number), which row 99 (-4.9) is within 1.5 rows of
    _, ver = om.gen_ticks(frame, [], [("Multiple", 0.0, 2.5, 6, True), ("Single", 0.0, 9, False)], az, el)
    assert {y: (t["label"], t["size"]) for y, t in ver.items()} == {25: ("2.5", 6), 50: ("0.0", 9), 75: ("-2.5", 6), 99: ("-5.0", 6)}
    ordered = om.ticks_sorted(hor, ver)
    assert [(t["vertical"], t["pos"]) for t in ordered] == [(False, 0), (False, 50), (False, 100), (False, 150), (True, 25), (True, 50), (True, 75), (True, 99)]


def test_layers_are_drawn_in_the_order_of_output_image():
    w, h = 40, 20
    az, el = fast_frame(10.0, 20.0, w, h)
    frame = {"direction": 10.0, "fov": 20.0, "width": w, "height": h, "tilt": 0.0}
    img = np.full((h, w, 3), 7, dtype=np.uint8)
    out, ticks, info = om.draw_overlay(img, frame, [("Single", 10.0, 30, False)], [("Single", 0.0, 25, False)], True, 0.0, az, el)
    assert info["eye_y"] == [10] * w and info["flat_y"] == [10] * w and info["steepest"] == 0
    assert (out[10, :] == om.EYE_LEVEL_COLOR).all()            # eye level last: over the flat horizon and both ticks
    assert (out[:10, 20] == om.WHITE).all() and (out[11:, 20] == om.WHITE).all()  # the tick of size 30 > h is cut at the border
    assert (img == 7).all() and len(ticks) == 2
    out, _, _ = om.draw_overlay(img, frame, [], [("Single", 0.0, 25, False)], False, 0.0, az, el)
    assert (out[10, :] == om.FLAT_HORIZON_COLOR).all()         # the flat horizon over the vertical tick
    out, _, _ = om.draw_overlay(img, frame, [], [("Single", 0.0, 25, False)], False, None, az, el)
    assert (out[10, :26] == om.WHITE).all() and (out[10, 26:] == 7).all()
