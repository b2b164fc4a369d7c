"""The last stage of InterpolatingRectilinearGenerator::generate as the reference writes it — a model of what atmrt_debug_interp_blend
must return, written from interpolating_rectilinear.rs and generators/mod.rs and from nothing under oracle/ or csrc/.

Python floats are IEEE doubles and every operator rounds once, which is how un-annotated Rust computes: an expression copied from the
reference operator by operator gives the reference's bits.  The mask dispatch is the reference's match over [Option; 4] (Some / None
patterns), not a table of bit masks, so that a typo cannot be shared with the kernel.

    cache_coords                :186-204      FovData::cache_coords
    collect_trace_points        :213-243
    match_sequence              :245-265
    interpolate_trace_points    :267-337      and its helpers :339-393
    TracePoint.interpolate      generators/mod.rs:33-43, PixelColor.interpolate :68-79, Color::interpolate object/mod.rs:148-155
    interpolate                 :395-418      the pixel: the groups that give a point, and the four-corner angle blend
    blend                       generate :127-155 over an image, with the lattice standing in for Cache::get_pixel, and the step count

A census (Census) can be handed to blend(): it records which arm of the match every group took, whether it gave a point, and on
which side of 0.5 every comparison fell.  tests/test_interp_blend_model.py asserts on it that the cases reach what they claim."""
import math
from collections import namedtuple

import numpy as np

TERRAIN, RGBA = 0, 1  # atmrt_color_tag

# PixelColor: Terrain(alpha) or Rgba(Color {r, g, b, a})
Terrain = namedtuple("Terrain", "alpha")
Rgba = namedtuple("Rgba", "r g b a")
TracePoint = namedtuple("TracePoint", "lat lon distance elevation path_length normal color")  # normal: (x, y, z)
ResultPixel = namedtuple("ResultPixel", "elevation_angle azimuth trace_points")
Indexed = namedtuple("Indexed", "index value")
Some = namedtuple("Some", "value")  # Option<T>: Some(value) or None

SEQUENCE = ((0, 0), (0, 1), (1, 0), (1, 1))


class Census:
    """groups: [(mask, accepted)] with mask = sum of 1 << corner over the corners present; sides[(arm, site)] = the set of
    sign(value - 0.5) over the evaluations of that comparison, arm = the mask of the match arm it belongs to."""

    def __init__(self):
        self.groups = []
        self.sides = {}
        self.pixel_totals = []   # corner points together, per pixel
        self.pixel_groups = []   # groups, per pixel

    def side(self, arm, site, value):
        self.sides.setdefault((arm, site), set()).add((value > 0.5) - (value < 0.5))


_census = None
_arm = 0


def _lt_half(site, value):  # value < 0.5
    if _census is not None:
        _census.side(_arm, site, value)
    return value < 0.5


def _ge_half(site, value):  # value >= 0.5
    if _census is not None:
        _census.side(_arm, site, value)
    return value >= 0.5


def as_i32(v):
    """Rust `f64 as i32`: towards zero, saturating, NaN -> 0."""
    if v != v:
        return 0
    if v <= -2147483648.0:
        return -2147483648
    if v >= 2147483647.0:
        return 2147483647
    return int(v)


def floor(v):
    return float(math.floor(v)) if math.isfinite(v) else v


def cache_coords(elevation, direction, min_elev_step, min_dir_step):  # :186-204
    elev_index_f = elevation / min_elev_step
    dir_index_f = direction / min_dir_step
    elev_index = as_i32(floor(elev_index_f))
    dir_index = as_i32(floor(dir_index_f))
    rem_elev = elev_index_f - float(elev_index)
    rem_dir = dir_index_f - float(dir_index)
    return [(elev_index + i, dir_index + j) for i, j in SEQUENCE], rem_elev, rem_dir


def same_class(a, b):  # generators/mod.rs:60-66
    return (isinstance(a, Terrain) and isinstance(b, Terrain)) or (isinstance(a, Rgba) and isinstance(b, Rgba))


def color_interpolate(a, b, coeff):  # generators/mod.rs:68-79
    if isinstance(a, Terrain) and isinstance(b, Terrain):
        return Terrain(a.alpha * (1.0 - coeff) + b.alpha * coeff)
    if isinstance(a, Rgba) and isinstance(b, Rgba):  # Color::interpolate, object/mod.rs:148-155
        return Rgba(a.r * (1.0 - coeff) + b.r * coeff, a.g * (1.0 - coeff) + b.g * coeff, a.b * (1.0 - coeff) + b.b * coeff,
                    a.a * (1.0 - coeff) + b.a * coeff)
    # The two mixed arms.  No case can reach them: collect_trace_points only groups points of the same class, and only points of one
    # group are ever interpolated.  They are here because the reference has them; no test asks for them.
    if isinstance(a, Terrain):
        return Terrain(a.alpha)
    return Terrain(b.alpha)


def tp_interpolate(a, b, coeff):  # generators/mod.rs:33-43
    return TracePoint(
        lat=a.lat * (1.0 - coeff) + b.lat * coeff,
        lon=a.lon * (1.0 - coeff) + b.lon * coeff,
        distance=a.distance * (1.0 - coeff) + b.distance * coeff,
        elevation=a.elevation * (1.0 - coeff) + b.elevation * coeff,
        path_length=a.path_length * (1.0 - coeff) + b.path_length * coeff,
        normal=tuple(p * (1.0 - coeff) + q * coeff for p, q in zip(a.normal, b.normal)),
        color=color_interpolate(a.color, b.color, coeff))


def collect_trace_points(pixels, step_size):  # :213-243
    result = []
    for index, pixel in zip(SEQUENCE, pixels):
        for trace_point in pixel.trace_points:
            close = next((idx for idx, points in enumerate(result)
                          if any(abs(trace_point.distance - point.value.distance) < step_size
                                 and same_class(trace_point.color, point.value.color) for point in points)), None)
            if close is not None:
                result[close].append(Indexed(index, trace_point))
            else:
                result.append([Indexed(index, trace_point)])
    return result


def match_sequence(vals):  # :245-265
    result = [None, None, None, None]
    for val in vals:
        match val.index:
            case (0, 0):
                result[0] = Some(val.value)
            case (0, 1):
                result[1] = Some(val.value)
            case (1, 0):
                result[2] = Some(val.value)
            case (1, 1):
                result[3] = Some(val.value)
            case _:
                raise AssertionError("unreachable")
    return result


def interpolate_two_adjacent(elem0, elem1, rem_elev, rem_dir):  # :339-350
    if _ge_half("adjacent.rem_elev>=", rem_elev):
        return None
    return tp_interpolate(elem0, elem1, rem_dir)


def interpolate_two_diagonal(elem0, elem1, rem_elev, rem_dir):  # :352-364
    if (_ge_half("diagonal.rem_elev>=", rem_elev) and _lt_half("diagonal.rem_dir<", rem_dir)) or \
            (_lt_half("diagonal.rem_elev<", rem_elev) and _ge_half("diagonal.rem_dir>=", rem_dir)):
        return None
    coeff = rem_elev * rem_dir / (rem_elev * rem_dir + (1.0 - rem_elev) * (1.0 - rem_dir))
    return tp_interpolate(elem0, elem1, coeff)


def interpolate_three(elem0, elem1, elem2, rem_elev, rem_dir):  # :366-380
    if _ge_half("three.rem_elev>=", rem_elev) and _ge_half("three.rem_dir>=", rem_dir):
        return None
    sum_ = 1.0 - rem_elev + rem_elev * (1.0 - rem_dir)
    interp = tp_interpolate(elem0, elem1, rem_dir)
    return tp_interpolate(interp, elem2, rem_elev * (1.0 - rem_dir) / sum_)


def interpolate_four(elem0, elem1, elem2, elem3, rem_elev, rem_dir):  # :382-393
    interp1 = tp_interpolate(elem0, elem1, rem_dir)
    interp2 = tp_interpolate(elem2, elem3, rem_dir)
    return tp_interpolate(interp1, interp2, rem_elev)


def interpolate_trace_points(points, rem_elev, rem_dir):  # :267-337
    global _arm
    present_elems = match_sequence(points)
    _arm = sum(1 << k for k, e in enumerate(present_elems) if e is not None)  # for the census only
    match present_elems:
        case [None, None, None, None]:
            return None
        case [Some(elem), None, None, None]:
            if _lt_half("single.rem_elev<", rem_elev) and _lt_half("single.rem_dir<", rem_dir):
                return elem
            return None
        case [None, Some(elem), None, None]:
            if _lt_half("single.rem_elev<", rem_elev) and _ge_half("single.rem_dir>=", rem_dir):
                return elem
            return None
        case [None, None, Some(elem), None]:
            if _ge_half("single.rem_elev>=", rem_elev) and _lt_half("single.rem_dir<", rem_dir):
                return elem
            return None
        case [None, None, None, Some(elem)]:
            if _ge_half("single.rem_elev>=", rem_elev) and _ge_half("single.rem_dir>=", rem_dir):
                return elem
            return None
        case [Some(elem0), Some(elem1), None, None]:
            return interpolate_two_adjacent(elem0, elem1, rem_elev, rem_dir)
        case [Some(elem0), None, Some(elem1), None]:
            return interpolate_two_adjacent(elem0, elem1, rem_dir, rem_elev)
        case [Some(elem0), None, None, Some(elem1)]:
            return interpolate_two_diagonal(elem0, elem1, rem_elev, rem_dir)
        case [None, Some(elem0), Some(elem1), None]:
            return interpolate_two_diagonal(elem0, elem1, rem_elev, 1.0 - rem_dir)
        case [None, Some(elem0), None, Some(elem1)]:
            return interpolate_two_adjacent(elem0, elem1, 1.0 - rem_dir, rem_elev)
        case [None, None, Some(elem0), Some(elem1)]:
            return interpolate_two_adjacent(elem0, elem1, 1.0 - rem_elev, rem_dir)
        case [Some(elem0), Some(elem1), Some(elem2), None]:
            return interpolate_three(elem0, elem1, elem2, rem_elev, rem_dir)
        case [Some(elem0), Some(elem1), None, Some(elem2)]:
            return interpolate_three(elem1, elem0, elem2, rem_elev, 1.0 - rem_dir)
        case [Some(elem0), None, Some(elem1), Some(elem2)]:
            return interpolate_three(elem0, elem2, elem1, 1.0 - rem_elev, rem_dir)
        case [None, Some(elem0), Some(elem1), Some(elem2)]:
            return interpolate_three(elem2, elem1, elem0, 1.0 - rem_elev, 1.0 - rem_dir)
        case [Some(elem0), Some(elem1), Some(elem2), Some(elem3)]:
            return interpolate_four(elem0, elem1, elem2, elem3, rem_elev, rem_dir)
    raise AssertionError("unreachable")


def interpolate(pixels, rem_elev, rem_dir, step_size):  # :395-418
    assert len(pixels) == 4
    groups = collect_trace_points(pixels, step_size)
    trace_points = []
    for points in groups:
        tp = interpolate_trace_points(points, rem_elev, rem_dir)
        if _census is not None:
            _census.groups.append((_arm, tp is not None))
        if tp is not None:
            trace_points.append(tp)
    if _census is not None:
        _census.pixel_totals.append(sum(len(p.trace_points) for p in pixels))
        _census.pixel_groups.append(len(groups))
    return ResultPixel(
        elevation_angle=pixels[0].elevation_angle * (1.0 - rem_elev) * (1.0 - rem_dir)
        + pixels[1].elevation_angle * (1.0 - rem_elev) * rem_dir
        + pixels[2].elevation_angle * rem_elev * (1.0 - rem_dir)
        + pixels[3].elevation_angle * rem_elev * rem_dir,
        azimuth=pixels[0].azimuth * (1.0 - rem_elev) * (1.0 - rem_dir)
        + pixels[1].azimuth * (1.0 - rem_elev) * rem_dir
        + pixels[2].azimuth * rem_elev * (1.0 - rem_dir)
        + pixels[3].azimuth * rem_elev * rem_dir,
        trace_points=trace_points)


# ---- the lattice and the image: the arrays atmrt_debug_interp_blend takes and returns ---------------------------------------------
def lattice_pixels(lattice):
    """[ne][nd] ResultPixel of the lattice dict (the layout of atmrt_interp_lattice_t)."""
    count = np.asarray(lattice["hit_count"])
    ne, nd = count.shape
    f = {k: np.asarray(lattice[k], dtype=np.float64).tolist() for k in ("lat", "lon", "distance", "elevation", "path_length")}
    normal, rgba = np.asarray(lattice["normal"], dtype=np.float64).reshape(-1, 3).tolist(), np.asarray(lattice["rgba"], dtype=np.float64).reshape(-1, 4).tolist()
    tag = np.asarray(lattice["color_tag"]).tolist()
    az, el = np.asarray(lattice["azimuth"], dtype=np.float64).tolist(), np.asarray(lattice["elevation_angle"], dtype=np.float64).tolist()
    rows, k = [], 0
    for i in range(ne):
        row = []
        for j in range(nd):
            tps = []
            for _ in range(int(count[i, j])):
                color = Terrain(rgba[k][3]) if tag[k] == TERRAIN else Rgba(*rgba[k])
                tps.append(TracePoint(f["lat"][k], f["lon"][k], f["distance"][k], f["elevation"][k], f["path_length"][k], tuple(normal[k]), color))
                k += 1
            row.append(ResultPixel(el[i][j], az[i][j], tps))
        rows.append(row)
    assert k == len(tag)
    return rows


def blend(case, census=None):
    """generate :127-155 for the image of `case` (elev, dir [h][w]; min_elev_step, min_dir_step, simulation_step; lattice) as the
    arrays of a ResultPixels, plus ray_steps = the px_steps of every lattice point some pixel references, each once (the reference's
    cache computes exactly those).  The lattice must be the bounding rectangle of the referenced points: anything else raises."""
    global _census
    elev, dirs = np.asarray(case["elev"], dtype=np.float64), np.asarray(case["dir"], dtype=np.float64)
    h, w = elev.shape
    coords = [[cache_coords(float(elev[y, x]), float(dirs[y, x]), case["min_elev_step"], case["min_dir_step"]) for x in range(w)] for y in range(h)]
    keys = [pt for row in coords for c in row for pt in c[0]]
    ei0, di0 = min(k[0] for k in keys), min(k[1] for k in keys)
    ne, nd = max(k[0] for k in keys) - ei0 + 1, max(k[1] for k in keys) - di0 + 1
    pixels = lattice_pixels(case["lattice"])
    if (len(pixels), len(pixels[0])) != (ne, nd):
        raise ValueError(f"the rays reference {ne} x {nd} lattice points, the lattice has {len(pixels)} x {len(pixels[0])}")
    out = {"width": w, "height": h, "azimuth": np.zeros((h, w)), "elevation_angle": np.zeros((h, w)), "hit_count": np.zeros((h, w), dtype=np.uint32)}
    tps, referenced = [], set()
    _census = census
    try:
        for y in range(h):
            for x in range(w):
                points_to_read, rem_elev, rem_dir = coords[y][x]
                referenced.update(points_to_read)
                px = interpolate([pixels[e - ei0][d - di0] for e, d in points_to_read], rem_elev, rem_dir, case["simulation_step"])
                out["azimuth"][y, x], out["elevation_angle"][y, x], out["hit_count"][y, x] = px.azimuth, px.elevation_angle, len(px.trace_points)
                tps.extend(px.trace_points)
    finally:
        _census = None
    n = len(tps)
    out["n_hits"] = n
    out["hit_offset"] = (np.cumsum(out["hit_count"].ravel(), dtype=np.uint64) - out["hit_count"].ravel()).reshape(h, w).astype(np.uint64)
    for k in ("lat", "lon", "distance", "elevation", "path_length"):
        out[k] = np.array([getattr(t, k) for t in tps], dtype=np.float64)
    out["normal"] = np.array([t.normal for t in tps], dtype=np.float64).reshape(n, 3)
    out["color_tag"] = np.array([TERRAIN if isinstance(t.color, Terrain) else RGBA for t in tps], dtype=np.uint32)
    # Terrain(alpha) is {0, 0, 0, alpha} in the flattened result (include/atmrt.h, atmrt_result_t.rgba)
    out["rgba"] = np.array([(0.0, 0.0, 0.0, t.color.alpha) if isinstance(t.color, Terrain) else tuple(t.color) for t in tps], dtype=np.float64).reshape(n, 4)
    px_steps = np.asarray(case["lattice"]["px_steps"])
    out["ray_steps"] = sum(int(px_steps[e - ei0, d - di0]) for e, d in referenced)
    out["keys"] = np.array([[c[0][0] for c in row] for row in coords], dtype=np.int64)  # (elev_index, dir_index) per pixel
    out["rems"] = np.array([[(c[1], c[2]) for c in row] for row in coords], dtype=np.float64)
    return out


FIELDS = ("hit_count", "hit_offset", "azimuth", "elevation_angle", "lat", "lon", "distance", "elevation", "path_length", "normal", "color_tag", "rgba")


def differences(got, want):
    """Names of the outputs of `got` (a ResultPixels) that are not, bit for bit, those of `want` (blend())."""
    bad = [k for k in FIELDS if np.asarray(got[k]).shape != np.asarray(want[k]).shape or np.asarray(got[k]).tobytes() != np.asarray(want[k]).astype(np.asarray(got[k]).dtype).tobytes()]
    return bad + [k for k in ("n_hits", "ray_steps") if int(got[k]) != int(want[k])]


_results = {}


def expected(case):
    """(blend(case), its Census), computed once per process and shared by the tests: do not change them."""
    if case["name"] not in _results:
        census = Census()
        _results[case["name"]] = (blend(case, census), census)
    return _results[case["name"]]
