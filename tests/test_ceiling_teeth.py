"""Proof, on the CPU, that the ground of tests/ceiling_cases.py has teeth: a terrain ceiling table (csrc/atmrt_ceiling.h) read one
row or one bin beside the right entry is wrong there, both entry by entry (the table of tests/csrc/ceiling_host.cpp against the
oracle's terrain) and pixel by pixel (tests/ceiling_model.py: the march's use of the table, restated over the oracle's rays,
geodesic points and terrain).  The frames of tests/test_gpu_ceiling_table.py are these views: a kernel that took the neighbouring
row or bin would not match the oracle there.  On the level-1 terrain of the other GPU tests no bin slip shows at all."""
import numpy as np
import pytest

import ceiling_cases as cc
import ceiling_model
import escape_cases
import test_ceiling_host as host
from oracle_binding import Oracle
from util import run_oracle


@pytest.fixture(scope="module")
def exe():
    return host._exe("ceiling_host", ["-O2"])


@pytest.fixture(scope="module")
def oracle():
    return Oracle("det")


def _violations(oracle, tiles, r):
    """The interior samples (seeded directions inside their bin, no border row or bin) of a host run, looked up through the oracle:
    count(plane, rows, bins) = how many lie above plane[step + rows][bin + bins] less the table's 1 m margin."""
    rows, bins = r["cell"].shape[0], r["cell"].shape[1] - 1
    i, j, k = r["where"].T
    keep = (k >= 4) & (i >= 1) & (i < rows - 1) & (j >= 1) & (j < bins - 1)
    t = oracle.terrain_new(tiles)
    try:
        ground = np.array([oracle.get_elev(t, lat, lon) or 0.0 for lat, lon in r["samples"][keep, :2]])
    finally:
        oracle.terrain_free(t)
    i, j = i[keep], j[keep]
    return len(ground), lambda plane, di=0, dj=0: int((ground > plane[i + di, j + dj] - 1.0 + 1e-6).sum())


def test_the_table_has_teeth_on_spikes(exe, oracle, tmp_path):
    """The view of the table tests (46.5 N 8.5 E, yaw 45, fov 12, 64 x 32, step 100 m, reach 30 km: 301 rows x 82 bins, 71,760
    interior samples), every sample against the entry it would read if the table were off by one.  Measured:

        tile                      own  row + 1  row - 1  bin + 1  bin - 1  suffix own  suffix of row + 1
        dense  (seed 11, 2 %)       0     3243     3246      213      186           0                 10
        sparse (seed 11, 0.1 %)     0      311      325       15       28           0                 49

    (15 % of the sparse tile's suffix entries are 1 m.)  Every off-by-one count must be above 0; at least 10 makes the tiles fit
    for the purpose, so that no single lucky sample carries the GPU tests."""
    for which in ("dense", "sparse"):
        tiles = cc.tile(which)
        r = host._run(exe, tmp_path, tiles, *cc.OBSERVER, cc.YAW, cc.STEP, cc.REACH)
        n, count = _violations(oracle, tiles, r)
        cells = {name: count(r["cell"], *shift) for name, shift in cc.SHIFTS.items()}
        own, suffix_own, suffix_next = count(r["cell"]), count(r["suffix"]), count(r["suffix"], 1, 0)
        print(f"\n{which}: {n} interior samples, own {own}, {cells}, suffix own {suffix_own}, suffix of row + 1 {suffix_next}, "
              f"{(r['suffix'][:, :-1] == 1.0).mean():.3f} of the suffix entries are 1 m")
        assert n > 70_000 and own == 0 and suffix_own == 0
        if which == "dense":
            assert all(v >= 10 for v in cells.values()), cells
        else:
            assert suffix_next >= 10, suffix_next


def _view(oracle, exe, tmp_path, name, columns):
    lib = escape_cases.load_lib()
    v = cc.VIEWS[name]
    cfg, tiles = cc.config(name), cc.tile(v["tile"])
    want = run_oracle(oracle, cfg, tiles)
    r = host._run(exe, tmp_path, tiles, *cc.OBSERVER, cc.YAW, v["step"], v["reach"], tilt=v["tilt"], per_cell=-4)
    # Frame::ceil_floor (prepare_ceiling): the certificate from the lowest value an entry can have, 1 m, less a step; plus a step
    floor = escape_cases.certificate(lib, None, cc.RADIUS, cfg.params.wavelength, 1.0, v["step"])[1] + v["step"]
    frame = ceiling_model.Frame(oracle, cfg, tiles, want, columns, v["altitude"])
    return frame, r, floor


def _changed(frame, r, floor, first, cell=(0, 0), suffix=(0, 0)):
    got = frame.march(r["layout"], cc.shifted(r["cell"], *cell), cc.shifted(r["suffix"], *suffix), floor)
    return int((got[0] != first).sum()), int((got[1] != frame.left).sum())


@pytest.mark.parametrize("name,columns", [("near", range(0, cc.W, 4)), ("far", range(cc.W)), ("up", range(0, cc.W, 2))])
def test_the_frames_have_teeth_on_spikes(exe, oracle, tmp_path, name, columns):
    """With the host's table the model reproduces the oracle's hit / miss and the step of the first crossing in every modelled
    pixel (all rows of the stated columns); with the table shifted, pixels change.  Measured (changed pixels of the modelled ones):

        view  modelled  hits  rays that leave  row + 1  row - 1  bin + 1  bin - 1  suffix row + 1  suffix row + 2
        near       512   466               14      207      359        0       12   0 (12 leave elsewhere)      0
        far       2048  1456              571     1106      943       61       60   0 (364)                     0
        up        1024   541              483      506      524        1       13   0 (405)                    43

    near is the view of the table tests; its bins are 26 - 78 m wide, hardly more than the cover's two posts of 31 m, so a slip of
    one bin changes few pixels there and the far view (300 steps of 200 m) carries it.

    THE SUFFIX PLANE SHIFTED BY ONE ROW CHANGES NO PIXEL, ON ANY GROUND: march_steps tests the crossing of step i before it lets the
    ray leave at step i, and suffix[i + 1] bounds every sample after i, so a march that read the suffix of the next row would
    still be right (and one that read the previous row's, which is never lower, only leaves later).  What such a slip changes is
    the step at which rays leave (asserted: at least 10), i.e. the work.  The smallest slip of the suffix that loses a hit is two
    rows, and the up view shows it."""
    frame, r, floor = _view(oracle, exe, tmp_path, name, columns)
    first, frame.left, lookups = frame.march(r["layout"], r["cell"], r["suffix"], floor)
    ok = frame.agrees_with_the_oracle(first)
    hits, leave = int((first >= 0).sum()), int((frame.left >= 0).sum())
    print(f"\n{name}: {len(first)} pixels, {hits} hits, {leave} rays leave, {int(lookups.sum())} lookups of {frame.h.size} samples")
    assert ok.all(), (int((~ok).sum()), np.flatnonzero(~ok)[:10])
    assert 0 < hits < len(first) and lookups.sum() < 0.2 * frame.h.size  # rays pass between the spikes, most samples are skipped
    figures = {k: _changed(frame, r, floor, first, cell=s, suffix=s)[0] for k, s in cc.SHIFTS.items()}
    one = _changed(frame, r, floor, first, suffix=(1, 0))
    two = _changed(frame, r, floor, first, suffix=(2, 0))
    print(f"  changed pixels: {figures}, suffix row + 1 {one[0]} ({one[1]} rays leave elsewhere), suffix row + 2 {two[0]}")
    assert figures["row + 1"] >= 10 and figures["row - 1"] >= 10, figures
    assert one[0] == 0 and one[1] >= 10, one
    if name == "far":
        assert figures["bin + 1"] >= 10 and figures["bin - 1"] >= 10, figures
    if name == "up":
        assert leave >= 0.25 * len(first) and two[0] >= 10, (leave, two)
