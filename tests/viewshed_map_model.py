"""The viewshed-map rule of include/atmrt.h ("viewshed map") restated in numpy over any planes status, hidden, lat, lon.  Test
infrastructure only: what atmrt_viewshed_map* must write, plane for plane, and the stats of the call."""
import numpy as np

import viewshed_model as vm

PLANES = (("n_samples", np.uint32), ("n_seen", np.uint32), ("min_hidden", np.float64))
STATS = ("n_samples", "n_binned", "n_outside", "n_skipped", "n_seen")


def grid_tuple(grid):
    """(lat0, lon0, cell_lat, cell_lon, n_lat, n_lon) of a tuple or of anything with such attributes."""
    if isinstance(grid, (tuple, list)):
        return tuple(grid)
    return (grid.lat0, grid.lon0, grid.cell_lat, grid.cell_lon, grid.n_lat, grid.n_lon)


def cells(grid, lat, lon):
    """atmrt_geo_grid_cell: i * n_lon + j, -1 outside; the south and west edges belong to a cell, the north and east ones do not."""
    lat0, lon0, cell_lat, cell_lon, n_lat, n_lon = grid_tuple(grid)
    with np.errstate(invalid="ignore", over="ignore"):
        fi = np.floor((lat - np.float64(lat0)) / np.float64(cell_lat))
        fj = np.floor((lon - np.float64(lon0)) / np.float64(cell_lon))
        inside = (fi >= 0.0) & (fi < float(n_lat)) & (fj >= 0.0) & (fj < float(n_lon))
    return np.where(inside, np.where(inside, fi, 0.0).astype(np.int64) * int(n_lon) + np.where(inside, fj, 0.0).astype(np.int64), -1)


def bin_planes(grid, status, hidden, lat, lon, into=None):
    """-> (n_samples, n_seen, min_hidden, each [n_lat][n_lon], and the stats of this call).  into = (n_samples, n_seen, min_hidden) of a
    map on the same grid: accumulate (they are not changed; the sums and minima are returned)."""
    _, _, _, _, n_lat, n_lon = grid_tuple(grid)
    status = np.asarray(status).ravel().astype(np.int64)
    hidden, lat, lon = (np.asarray(a, dtype=np.float64).ravel() for a in (hidden, lat, lon))
    n_cells = int(n_lat) * int(n_lon)
    if into is None:
        n_samples, n_seen, min_hidden = np.zeros(n_cells, np.uint32), np.zeros(n_cells, np.uint32), np.full(n_cells, np.inf)
    else:
        n_samples, n_seen, min_hidden = (np.array(a).ravel().copy() for a in into)
    skipped = np.isnan(lat) | np.isnan(lon) | (status > 3)
    cell = np.where(skipped, -1, cells(grid, lat, lon))
    binned = cell >= 0
    seen = binned & ((status == vm.SEEN) | (status == vm.BELOW_FAN))
    part = binned & ((status == vm.SEEN) | (status == vm.HIDDEN)) & ~np.isnan(hidden) & ~np.signbit(hidden)
    np.add.at(n_samples, cell[binned], np.uint32(1))
    np.add.at(n_seen, cell[seen], np.uint32(1))
    np.minimum.at(min_hidden, cell[part], hidden[part])
    stats = dict(n_samples=int(status.size), n_binned=int(binned.sum()), n_outside=int((~skipped & ~binned).sum()), n_skipped=int(skipped.sum()),
                 n_seen=int(seen.sum()))
    shape = (int(n_lat), int(n_lon))
    return n_samples.reshape(shape), n_seen.reshape(shape), min_hidden.reshape(shape), stats


def assert_same(got, want, tag=""):
    """got: (n_samples, n_seen, min_hidden, stats) with arrays of any integer width for the counts; want: bin_planes' tuple.  Counts
    equal, min_hidden byte for byte, stats equal."""
    for k, (name, dtype) in enumerate(PLANES):
        g, w = np.ascontiguousarray(got[k]).view(dtype) if name != "min_hidden" else np.ascontiguousarray(got[k], dtype=dtype), want[k]
        assert g.shape == w.shape, (tag, name, g.shape, w.shape)
        bad = np.argwhere(g.view(np.uint64 if name == "min_hidden" else dtype) != w.view(np.uint64 if name == "min_hidden" else dtype))
        assert bad.size == 0, f"{tag} {name}: {len(bad)} of {g.size} cells differ, first at {bad[:5].tolist()}: {g[tuple(bad[:5].T)]} vs {w[tuple(bad[:5].T)]}"
    assert {k: int(got[3][k]) for k in STATS} == want[3], (tag, got[3], want[3])
