"""The annotations of renderer::output_image restated in numpy / plain Python, line by line from src/renderer/mod.rs:28-365 and
:416-431 of the reference — the checker of atmrt_overlay_resolve_ticks and atmrt_draw_overlay*.  It shares nothing with the
product but the reference's text and the line rule written down in DESIGN.md §6 (imageproc's draw_line_segment_mut is an absent
crate: Bresenham over the longer axis with an f32 error term, pixels outside the image skipped).

`pixels` of the reference is Vec<Vec<ResultPixel>>; here `azimuth` and `elevation_angle` are its [H][W] float64 planes.
`frame` is a dict {direction, tilt, fov, width, height}: params.view.frame and params.output.width / height.
Ticks are tuples as config._ticks produces them: ("Single", angle, size, labelled) / ("Multiple", bias, step, size, labelled).
"""
import math

import numpy as np

WHITE = (255, 255, 255)
FLAT_HORIZON_COLOR = (0, 128, 255)  # :427
EYE_LEVEL_COLOR = (255, 128, 255)   # :430


def diff_azimuth(az1, az2):  # :28-37
    diff = az1 - az2
    if diff < -180.0:
        return diff + 360.0
    if diff > 180.0:
        return diff - 360.0
    return diff


def _first_min(values):
    """Iterator::min_by: the FIRST of equal minima."""
    best, idx = None, 0
    for i, v in enumerate(values):
        if best is None or v < best:
            best, idx = v, i
    return idx


def azimuth_to_x(azimuth, row0):  # :39-59
    candidate = _first_min(abs(diff_azimuth(azimuth, float(a))) for a in row0)
    neighboring_idx = 1 if candidate == 0 else candidate - 1
    diff_per_pixel = abs(diff_azimuth(float(row0[candidate]), float(row0[neighboring_idx])))
    return candidate if abs(diff_azimuth(float(row0[candidate]), azimuth)) < diff_per_pixel * 1.5 else None


def elevation_to_y(elevation, col0):  # :61-80
    candidate = _first_min(abs(elevation - float(e)) for e in col0)
    neighboring_idx = 1 if candidate == 0 else candidate - 1
    diff_per_pixel = abs(float(col0[candidate]) - float(col0[neighboring_idx]))
    return candidate if abs(float(col0[candidate]) - elevation) < diff_per_pixel * 1.5 else None


def rust_round(x):
    """f64::round: half away from zero (Python's round() is banker's)."""
    return math.copysign(math.floor(abs(x) + 0.5), x) if abs(x) < 2.0 ** 52 else x


def num_decimals(x):  # :208-216
    for i in range(10):
        mul_x = x * 10.0 ** i
        if abs(rust_round(mul_x) - mul_x) < 0.001:
            return i
    return 10


def tick_angle(tick):  # TickLike::angle, params.rs:347-352, 379-384: the angle of a Single, the STEP of a Multiple
    return tick[1] if tick[0] == "Single" else tick[2]


def tick_labelled(tick):
    return tick[-1]


def round_decimals(ticks):  # :218-225
    return max([num_decimals(tick_angle(t)) for t in ticks if tick_labelled(t)], default=0)


def fmt(angle, decimals):
    """format!("{:.1$}", angle, decimals): correctly rounded from the binary value, sign kept on a negative zero result."""
    return format(angle, f".{decimals}f")


def into_draw_ticks(tick, frame, row0, decimals):  # :82-140
    out = []
    if tick[0] == "Single":
        _, azimuth, size, labelled = tick
        x = azimuth_to_x(azimuth, row0)
        if x is not None:
            out.append((x, {"size": size, "labelled": labelled, "label": fmt(azimuth, decimals)}))
        return out
    _, bias, step, size, labelled = tick
    min_az = frame["direction"] - frame["fov"] / 2.0
    max_az = frame["direction"] + frame["fov"] / 2.0
    current_az = math.ceil((min_az - bias) / step) * step + bias
    while current_az < max_az:
        if current_az < 0.0:
            azimuth = current_az + 360.0
        elif current_az >= 360.0:
            azimuth = current_az - 360.0
        else:
            azimuth = current_az
        x = azimuth_to_x(current_az, row0)  # the UNWRAPPED value (:125)
        if x is not None:
            out.append((x, {"size": size, "labelled": labelled, "label": fmt(azimuth, decimals)}))
        current_az += step
    return out


def into_draw_ticks_vertical(tick, frame, col0, decimals):  # :142-201
    out = []
    if tick[0] == "Single":
        _, elevation, size, labelled = tick
        y = elevation_to_y(elevation, col0)
        if y is not None:
            out.append((y, {"size": size, "labelled": labelled, "label": fmt(elevation, decimals)}))
        return out
    _, bias, step, size, labelled = tick
    aspect = float(frame["height"]) / float(frame["width"])
    min_elev = frame["tilt"] - frame["fov"] * aspect / 2.0
    max_elev = frame["tilt"] + frame["fov"] * aspect / 2.0
    current_elev = math.ceil((min_elev - bias) / step) * step + bias
    while current_elev < max_elev:
        if current_elev < -90.0:
            elevation = -180.0 - current_elev
        elif current_elev > 90.0:
            elevation = 180.0 - current_elev
        else:
            elevation = current_elev
        y = elevation_to_y(elevation, col0)  # the FOLDED value (:186)
        if y is not None:
            out.append((y, {"size": size, "labelled": labelled, "label": fmt(elevation, decimals)}))
        current_elev += step
    return out


def gen_ticks(frame, ticks, vertical_ticks, azimuth, elevation_angle):  # :227-268
    """-> (horizontal {x: tick}, vertical {y: tick}).  A position taken twice keeps the larger size, the earlier one when equal."""
    row0 = np.asarray(azimuth)[0, :]
    col0 = np.asarray(elevation_angle)[:, 0]
    horizontal, vertical = {}, {}
    hd, vd = round_decimals(ticks), round_decimals(vertical_ticks)
    for tick in ticks:
        for x, t in into_draw_ticks(tick, frame, row0, hd):
            if x not in horizontal or horizontal[x]["size"] < t["size"]:
                horizontal[x] = t
    for tick in vertical_ticks:
        for y, t in into_draw_ticks_vertical(tick, frame, col0, vd):
            if y not in vertical or vertical[y]["size"] < t["size"]:
                vertical[y] = t
    return horizontal, vertical


def ticks_sorted(horizontal, vertical):
    """The library's order: by (vertical, pos)."""
    out = [dict(pos=x, vertical=False, **horizontal[x]) for x in sorted(horizontal)]
    return out + [dict(pos=y, vertical=True, **vertical[y]) for y in sorted(vertical)]


def segment_pixels(x0, y0, x1, y1):
    """The line rule: every pixel of the segment, in drawing order, before clipping."""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x0 > x1:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx = np.float32(x1 - x0)
    dy = np.float32(abs(y1 - y0))
    error = dx / np.float32(2.0)
    ystep = 1 if y0 < y1 else -1
    y = y0
    out = []
    for x in range(x0, x1 + 1):
        out.append((y, x) if steep else (x, y))
        error = np.float32(error - dy)
        if error < 0:
            y += ystep
            error = np.float32(error + dx)
    return out


def draw_line_segment(img, start, end, color):
    """imageproc::draw_line_segment_mut as DESIGN.md §6 pins it; pixels outside the image are skipped."""
    h, w = img.shape[:2]
    for x, y in segment_pixels(int(start[0]), int(start[1]), int(end[0]), int(end[1])):
        if 0 <= x < w and 0 <= y < h:
            img[y, x] = color


def draw_tick_lines(img, horizontal, vertical):  # draw_ticks, :285-322, without the text
    h, w = img.shape[:2]
    for x, tick in horizontal.items():
        draw_line_segment(img, (x, 0), (x, min(tick["size"], h)), WHITE)  # (the part beyond the image is skipped anyway)
    for y, tick in vertical.items():
        draw_line_segment(img, (0, y), (min(tick["size"], w), y), WHITE)


def find_elev(elevation_angle, column, elev):  # :325-343
    closest_elev = math.inf
    closest_elev_idx = 0
    for y in range(elevation_angle.shape[0]):
        e = float(elevation_angle[y, column])
        if abs(e - elev) < abs(closest_elev - elev):
            closest_elev = e
            closest_elev_idx = y
    neighbor = 1 if closest_elev_idx == 0 else closest_elev_idx - 1
    neighbor_elev = float(elevation_angle[neighbor, column])
    return closest_elev_idx if abs(closest_elev - elev) < abs(neighbor_elev - closest_elev) * 1.5 else None


def find_elev_all(elevation_angle, elev):
    """find_elev for every column, vectorised over the columns (the scan over y stays sequential with strict `<`)."""
    e = np.asarray(elevation_angle, dtype=np.float64)
    h, w = e.shape
    closest = np.full(w, np.inf)
    idx = np.zeros(w, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for y in range(h):
            better = np.abs(e[y] - elev) < np.abs(closest - elev)
            closest = np.where(better, e[y], closest)
            idx = np.where(better, y, idx)
        neighbor = np.where(idx == 0, 1, idx - 1)
        neighbor_elev = e[neighbor, np.arange(w)]
        found = np.abs(closest - elev) < np.abs(neighbor_elev - closest) * 1.5
    return [int(i) if f else None for i, f in zip(idx, found)]


def draw_const_elev(img, elevation_angle, elev, color):  # :345-365
    """Returns (y_of_x, the largest |y_new - y_old| of a drawn segment)."""
    ys = find_elev_all(elevation_angle, elev)
    steepest = 0
    maybe_y_old = ys[0]
    for x in range(1, img.shape[1]):
        maybe_y_new = ys[x]
        if maybe_y_old is not None and maybe_y_new is not None:
            draw_line_segment(img, (x - 1, maybe_y_old), (x, maybe_y_new), color)
            steepest = max(steepest, abs(maybe_y_new - maybe_y_old))
        maybe_y_old = maybe_y_new
    return ys, steepest


def draw_overlay(img, frame, ticks, vertical_ticks, show_eye_level, flat_horizon_deg, azimuth, elevation_angle):
    """output_image, :419-431, on a copy of img: ticks, then the flat horizon (flat_horizon_deg None: not drawn — the caller
    evaluates the condition of :420-422 and the angle of :424-426), then eye level.  Returns (image, ticks in the library's
    order, info)."""
    out = np.array(img, dtype=np.uint8, copy=True)
    horizontal, vertical = gen_ticks(frame, ticks, vertical_ticks, azimuth, elevation_angle)
    draw_tick_lines(out, horizontal, vertical)
    info = {"flat_y": None, "eye_y": None, "steepest": 0}
    if flat_horizon_deg is not None:
        info["flat_y"], s = draw_const_elev(out, elevation_angle, flat_horizon_deg, FLAT_HORIZON_COLOR)
        info["steepest"] = max(info["steepest"], s)
    if show_eye_level:
        info["eye_y"], s = draw_const_elev(out, elevation_angle, 0.0, EYE_LEVEL_COLOR)
        info["steepest"] = max(info["steepest"], s)
    return out, ticks_sorted(horizontal, vertical), info
