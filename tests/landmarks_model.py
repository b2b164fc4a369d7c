"""A brute-force numpy model of the landmark search (include/atmrt.h, atmrt_locate_landmarks*): the rule d2 = dlat * dlat +
dlon * dlon with dlat = lat - L.lat and dlon = (lon - L.lon) * L.lon_scale, every operation rounded on its own; within iff
d2 <= r2 = radius_deg * radius_deg; the winner is the within-point with the smallest d2, ties to the smallest flat pixel index, then
to the smallest point index inside the pixel.

Inputs are the arrays atmrt_generate returned for the frame (generators.ResultPixels), read through visibility_model.points /
skipped: the points a mode reads and the ones the search skips are the visibility map's."""
import numpy as np

import visibility_model as vm

HIT_DTYPE = np.dtype([("n_within", np.uint32), ("x", np.uint32), ("y", np.uint32), ("point", np.uint32), ("d2", np.float64),
                      ("distance", np.float64), ("elevation", np.float64)])
NONE = (0, 0xFFFFFFFF, 0xFFFFFFFF, 0, np.inf, np.nan, np.nan)


def d2(lm_lat, lm_lon, lm_scale, lat, lon):
    """The rule, broadcasting; NaN where the arithmetic says so."""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dlat = lat - lm_lat
        dlon = (lon - lm_lon) * lm_scale
        return dlat * dlat + dlon * dlon


def within(lm_lat, lm_lon, lm_scale, lat, lon, radius_deg):
    with np.errstate(invalid="ignore"):
        return d2(lm_lat, lm_lon, lm_scale, lat, lon) <= radius_deg * radius_deg  # NaN <= r2 is False


def landmark_arrays(landmarks):
    """A ctypes Landmark array (or a sequence of (lat, lon, lon_scale)) -> three float64 arrays."""
    rows = [(l.lat, l.lon, l.lon_scale) if hasattr(l, "lon_scale") else tuple(l) for l in landmarks]
    a = np.array(rows, dtype=np.float64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


def locate(res, landmarks, radius_deg, mode="first"):
    """-> (records [n] of HIT_DTYPE, stats dict without n_tested).  res needs hit_count, hit_offset [H][W], lat, lon, distance,
    elevation."""
    lat, lon, dist, pixel = vm.points(res, mode)
    cnt = res["hit_count"].ravel().astype(np.int64)
    off = res["hit_offset"].ravel().astype(np.int64)
    width = res["hit_count"].shape[1]
    if mode == "first":
        k = off[pixel]
        point = np.zeros(pixel.size, dtype=np.int64)
    else:
        point = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        k = np.repeat(off, cnt) + point
    elev = res["elevation"][k]
    skip = vm.skipped(lat, lon, dist)
    keep = np.flatnonzero(~skip)  # ascending (pixel, point): the first minimum of an argmin is the tie order's winner
    lm_lat, lm_lon, lm_scale = landmark_arrays(landmarks)
    out = np.empty(lm_lat.size, dtype=HIT_DTYPE)
    total = 0
    for i in range(lm_lat.size):
        v = d2(lm_lat[i], lm_lon[i], lm_scale[i], lat[keep], lon[keep])
        with np.errstate(invalid="ignore"):
            ok = v <= radius_deg * radius_deg
        n = int(ok.sum())
        total += n
        if n == 0:
            out[i] = NONE
            continue
        cand = np.flatnonzero(ok)
        w = keep[cand[np.argmin(v[cand])]]
        out[i] = (n, pixel[w] % width, pixel[w] // width, point[w], v[cand].min(), dist[w], elev[w])
    stats = {"n_points": int(lat.size), "n_skipped": int(skip.sum()), "n_within": total}
    return out, stats


def assert_records(got, want, tag=""):
    """Every field of every record, doubles by their bits (NaNs as one value)."""
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    for k in ("n_within", "x", "y", "point"):
        bad = np.flatnonzero(got[k] != want[k])
        assert bad.size == 0, (tag, k, bad.size, bad[:5], got[k][bad[:5]], want[k][bad[:5]])
    for k in ("d2", "distance", "elevation"):
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        gb, wb = g.view(np.uint64).copy(), w.view(np.uint64).copy()
        gb[np.isnan(g)] = wb[np.isnan(w)] = 0x7FF8000000000000
        bad = np.flatnonzero(gb != wb)
        assert bad.size == 0, (tag, k, bad.size, bad[:5], g[bad[:5]], w[bad[:5]])


def hand_made(lat, lon, dist, elev, cnt=None):
    """[H][W] planes -> the `res` dict of a frame with at most one point per pixel."""
    lat = np.asarray(lat, dtype=np.float64)
    h, w = lat.shape
    cnt = np.ones((h, w), dtype=np.uint32) if cnt is None else np.asarray(cnt)
    return {"hit_count": np.minimum(cnt, 1).astype(np.uint32), "hit_offset": np.arange(h * w, dtype=np.uint64).reshape(h, w),
            "lat": lat.ravel(), "lon": np.asarray(lon, dtype=np.float64).ravel(), "distance": np.asarray(dist, dtype=np.float64).ravel(),
            "elevation": np.asarray(elev, dtype=np.float64).ravel()}
