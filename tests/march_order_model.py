"""A numpy restatement of k_march_length_estimate (csrc/atmrt_kernels.hip) and of the contract of the counting sort behind it
(k_march_order_scan, k_march_order_scatter): the work queue of the whole-frame opaque march holds the frame's groups
of 64 consecutive pixels by ESTIMATED steps, longest first, and beside every group its estimate (Frame::ceil_order_steps), by which
the queue sizes its chunks and sets its priorities.  The estimate changes no bit of any frame, so only a restatement can see a wrong
stride, bin or row in it.

A group's estimate is the longest of four rays, the pixels min(64 g + 21 r, pixels - 1) for r = 0 .. 3.  A ray's height is the closed
form h(x) = alt + x slope + x^2 inv_2r over the distance table (slope = tan of its elevation angle, inv_2r = 1 / (2 * 7/6 * the
shape radius), 0 on a flat earth); its estimate is the first step i >= 1 at which ceiling_estimate_ends (csrc/atmrt_ceiling.h) holds
for the entry of row i of its bin — ascending and above the suffix, or below the cell — else the march's steps.

The device takes its own tan and may contract alt + x slope + x^2 inv_2r, so a comparison decided by less than H_MARGIN metres, or a
slope test by less than SLOPE_MARGIN, is not the model's to call: a group with such a decision at any step up to its estimate is
UNDECIDED.  1e-8 m is some three orders of magnitude above the rounding difference (1e-16 relative on a height of 6e4 m and a
distance of 2.5e5 m: 1e-11 m) and far below the spacing of the decisions: the table's entries are whole metres, h moves by metres
per step.  The expected share of undecided groups is therefore about (4 rays x 600 steps) x 2e-8 = 5e-5; the tests cap it at 1 %."""
import numpy as np

import ceiling_model

H_MARGIN = 1.0e-8       # metres
SLOPE_MARGIN = 1.0e-12  # of slope + 2 x inv_2r


def distance_table(step, reach):
    """the stepper's x: repeated addition, as ceiling_model.Frame builds it"""
    xs = [0.0]
    while xs[-1] + step <= reach:
        xs.append(xs[-1] + step)
    return np.array(xs)


def inv_2r(shape_radius):
    """1 / (2 R_eff), R_eff = 7/6 of the stepper's sphere; 0 for a flat earth (shape_radius None or 0)"""
    return 0.5 / (shape_radius * (7.0 / 6.0)) if shape_radius else 0.0


def sampled_pixels(n_pixels):
    """[groups][4] the pixels k_march_length_estimate takes its rays from"""
    n_groups = (n_pixels + 63) // 64
    return np.minimum(64 * np.arange(n_groups)[:, None] + 21 * np.arange(4)[None, :], n_pixels - 1)


def estimates(table, azimuth, elevation_angle, xs, altitude, inv_2r):
    """`table`: Context.debug_ceiling_table's dict (or the host builder's planes under the same keys); azimuth and elevation_angle:
    the frame's planes in degrees; xs: the distance table; altitude: the observer's resolved altitude.
    -> (estimate [groups] in 1 .. march_steps, undecided [groups])"""
    cell, suffix = np.asarray(table["cell"], dtype=np.float64), np.asarray(table["suffix"], dtype=np.float64)
    n_bins, steps = cell.shape[1] - 1, len(xs) - 1
    assert cell.shape[0] == steps + 1 and steps >= 1, (cell.shape, steps)
    px = sampled_pixels(azimuth.size)
    slope = np.tan(np.radians(np.asarray(elevation_angle, dtype=np.float64).ravel()[px]))  # [groups][4]
    bins = ceiling_model.bins_of(table["layout"], n_bins, np.asarray(azimuth, dtype=np.float64).ravel()[px])
    x = np.asarray(xs, dtype=np.float64)[1:]  # steps 1 .. march_steps
    h = altitude + x[None, None, :] * slope[:, :, None] + (x * x * inv_2r)[None, None, :]  # [groups][4][steps]
    rising = slope[:, :, None] + (2.0 * x * inv_2r)[None, None, :]
    rows = np.arange(1, steps + 1)
    ce = cell[rows[None, None, :], bins[:, :, None]]
    su = suffix[rows[None, None, :], bins[:, :, None]]
    ends = ((rising > 0.0) & (h > su)) | (h < ce)
    ray = np.where(ends.any(axis=2), ends.argmax(axis=2) + 1, steps)  # the first step that ends the ray, else march_steps
    estimate = ray.max(axis=1)
    close = (np.abs(h - su) < H_MARGIN) | (np.abs(h - ce) < H_MARGIN) | (np.abs(rising) < SLOPE_MARGIN)
    undecided = (close & (rows[None, None, :] <= estimate[:, None, None])).any(axis=(1, 2))
    return estimate.astype(np.int64), undecided


def undecided_cap(n_groups):
    """at most 1 % of a frame's groups, one group where it has fewer than 100"""
    return max(1, n_groups // 100)


def check_order(order, order_steps, estimate, undecided, steps):
    """The sort's contract and the estimates of the decided groups; returns a list of what is wrong (empty: nothing)."""
    order, order_steps = np.asarray(order, dtype=np.int64), np.asarray(order_steps, dtype=np.int64)
    n = estimate.size
    if order.size != n or order_steps.size != n:
        return [f"{order.size} entries of order, {order_steps.size} of order_steps, {n} groups"]
    wrong = []
    if not np.array_equal(np.sort(order), np.arange(n)):
        return ["order is no permutation of the groups"]
    if (np.diff(order_steps) > 0).any():
        wrong.append(f"order_steps increases at {np.flatnonzero(np.diff(order_steps) > 0)[:5].tolist()}")
    if order_steps.min() < 1 or order_steps.max() > steps:
        wrong.append(f"order_steps outside 1 .. {steps}: {int(order_steps.min())} .. {int(order_steps.max())}")
    if order_steps[0] != order_steps.max():
        wrong.append("order_steps[0] is not the maximum")
    bad = np.flatnonzero((order_steps != estimate[order]) & ~undecided[order])
    if bad.size:
        wrong.append(f"{bad.size} of {n} entries differ from the model, first (entry, group, device, model): "
                     f"{[(int(i), int(order[i]), int(order_steps[i]), int(estimate[order[i]])) for i in bad[:5]]}")
    if int(undecided.sum()) > undecided_cap(n):
        wrong.append(f"{int(undecided.sum())} of {n} groups undecided, more than {undecided_cap(n)}")
    return wrong
