"""A numpy model of the visibility map (include/atmrt.h, atmrt_visibility_map*): the binning rule, the trace points each mode
reads, the map with its statistics, the frame's bounds, and — FIRST mode — the number of runs the aggregating kernel may update.

Inputs are the arrays atmrt_generate returned for the frame (generators.ResultPixels): hit_count / hit_offset [H][W] and the hit
arrays lat, lon, distance in pixel order."""
import numpy as np

WAVE = 64


def grid_dict(grid):
    """A GeoGrid (ctypes) or a dict -> dict of plain Python numbers."""
    if isinstance(grid, dict):
        return grid
    return {k: getattr(grid, k) for k in ("lat0", "lon0", "cell_lat", "cell_lon", "n_lat", "n_lon")}


def cells(grid, lat, lon):
    """The binning rule: cell index i * n_lon + j of every point, -1 outside (NaN, infinities and huge values included)."""
    g = grid_dict(grid)
    lat, lon = np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fi = np.floor((lat - g["lat0"]) / g["cell_lat"])
        fj = np.floor((lon - g["lon0"]) / g["cell_lon"])
        inside = (fi >= 0) & (fi < g["n_lat"]) & (fj >= 0) & (fj < g["n_lon"])
    out = np.full(lat.shape, -1, dtype=np.int64)
    out[inside] = fi[inside].astype(np.int64) * g["n_lon"] + fj[inside].astype(np.int64)
    return out


def points(res, mode):
    """(lat, lon, distance, pixel) of the trace points a mode reads, in pixel order: "first" the first point of every pixel that has
    one, "all" every point."""
    cnt = res["hit_count"].ravel().astype(np.int64)
    off = res["hit_offset"].ravel().astype(np.int64)
    if mode == "first":
        pixel = np.flatnonzero(cnt > 0)
        k = off[pixel]
    else:
        pixel = np.repeat(np.arange(cnt.size), cnt)
        k = np.repeat(off, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return res["lat"][k], res["lon"][k], res["distance"][k], pixel


def skipped(lat, lon, dist):
    with np.errstate(invalid="ignore"):
        return np.isnan(lat) | np.isnan(lon) | np.isnan(dist) | (dist < 0)


def model_map(grid, lat, lon, dist):
    """-> (count uint32 [n_lat][n_lon], min_distance float64 with +inf in empty cells, stats without n_updates)."""
    g = grid_dict(grid)
    skip = skipped(lat, lon, dist)
    cell = cells(g, lat[~skip], lon[~skip])
    d = np.abs(dist[~skip])  # only -0.0 changes: it counts as 0.0
    inside = cell >= 0
    count = np.zeros(g["n_lat"] * g["n_lon"], dtype=np.uint32)
    mind = np.full(g["n_lat"] * g["n_lon"], np.inf)
    np.add.at(count, cell[inside], 1)
    np.minimum.at(mind, cell[inside], d[inside])
    stats = {"n_points": int(lat.size), "n_binned": int(inside.sum()), "n_outside": int((~inside).sum()), "n_skipped": int(skip.sum())}
    shape = (g["n_lat"], g["n_lon"])
    return count.reshape(shape), mind.reshape(shape), stats


def first_mode_runs(grid, res):
    """FIRST mode: maximal runs of equal valid cells within chunks of 64 consecutive pixels p = y * width + x (a pixel without a
    binned point ends a run): what the aggregating kernel may issue at most."""
    n_px = res["hit_count"].size
    lat, lon, dist, pixel = points(res, "first")
    per_pixel = np.full((n_px + WAVE - 1) // WAVE * WAVE, -1, dtype=np.int64)
    skip = skipped(lat, lon, dist)
    per_pixel[pixel[~skip]] = cells(grid, lat[~skip], lon[~skip])
    rows = per_pixel.reshape(-1, WAVE)
    head = rows >= 0
    head[:, 1:] &= rows[:, 1:] != rows[:, :-1]
    return int(head.sum())


def bounds(lat, lon, dist):
    """(lat_min, lat_max, lon_min, lon_max) over the points that are not skipped; all NaN when there is none."""
    keep = ~skipped(lat, lon, dist)
    if not keep.any():
        return (np.nan,) * 4
    return (np.nanmin(lat[keep]), np.nanmax(lat[keep]), np.nanmin(lon[keep]), np.nanmax(lon[keep]))
