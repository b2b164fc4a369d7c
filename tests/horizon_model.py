"""The horizon rule of include/atmrt.h ("horizon") restated in numpy over sight_model.Setting (the oracle's coords_at_dist, get_elev
and ray_paths of the deterministic flavour).  Test infrastructure only: what atmrt_horizon must write, record for record.  Every
formula below is written as the header states it, one IEEE operation at a time."""
import numpy as np

import sight_model as sm
import viewshed_model as vm

FOUND, ABOVE_FAN, BELOW_FAN = 0, sm.ABOVE_FAN, sm.BELOW_FAN
HORIZON_DTYPE = np.dtype([("status", np.int32), ("rounds_done", np.int32), ("k_star", np.int32), ("block_index", np.int32)] +
                         [(k, np.float64) for k in ("angle_clear", "angle_blocked", "resolution", "block_distance", "block_lat", "block_lon",
                                                    "block_elevation")])


def trace(H, T):
    """The rays H [n][m + 1] against the profile T [m + 1] -> (fails [n], block [n]): a ray is blocked at the first 1 <= i' <= m with
    c_{i'-1} * c_{i'} < 0.0 or H_{i'-1} < -1000 (block = i', else -1); it fails iff it is blocked or H_m is NaN."""
    m = H.shape[1] - 1
    at = vm.blocked_at(H, T)  # m + 1 where there is none
    block = np.where(at <= m, at, -1).astype(np.int32)
    return (block >= 0) | np.isnan(H[:, m]), block


def first_round(H, T, angles):
    """Round one over the K rays of the table -> (status, k*, block index of the failing ray of record, angle_clear, angle_blocked)."""
    K = H.shape[0]
    fails, block = trace(H, T)
    k = sm.pick(fails)  # one above the highest failing ray
    if k == K:
        return ABOVE_FAN, k, int(block[K - 1]), np.nan, angles[K - 1]
    if k == 0:
        return BELOW_FAN, k, -1, angles[0], np.nan
    return FOUND, k, int(block[k - 1]), angles[k], angles[k - 1]


def record(status, done, k_star, block, clear, blocked, resolution, d, lat, lon, T):
    rec = np.zeros((), dtype=HORIZON_DTYPE)
    rec["status"], rec["rounds_done"], rec["k_star"], rec["block_index"] = status, done, k_star, block
    rec["angle_clear"], rec["angle_blocked"], rec["resolution"] = clear, blocked, resolution
    if block >= 0:
        rec["block_distance"], rec["block_lat"], rec["block_lon"], rec["block_elevation"] = d[block], lat[block], lon[block], T[block]
    else:
        rec["block_distance"] = rec["block_lat"] = rec["block_lon"] = rec["block_elevation"] = np.nan
    return rec


def refine(heights, T, m, lo, hi, block, resolution, rounds):
    """Rounds 2 to `rounds` from the bracket [lo, hi]; heights(angles, m) -> H [64][m + 1].  -> (lo, hi, block, resolution, rounds_done)."""
    done = 1
    for r in range(1, rounds):
        e = sm.fan_angles(lo, hi)
        fails, blk = trace(heights(e, m), T)
        k = sm.pick(fails)
        done = r + 1
        if k in (0, 64):  # discarded: the bracket stays; the failing ray of record is this round's ray 0
            block = int(blk[0])
            break
        resolution = (hi - lo) / np.float64(63.0)
        lo, hi, block = e[k - 1], e[k], int(blk[k - 1])
    return lo, hi, block, resolution, done


def solve_one(setting, az, reach, angles, delta, H, rounds):
    """One azimuth against the shared table H [K][m + 1] of the first fan's `angles` -> a record."""
    d, m, lat, lon, T = setting.profile(az, reach)
    status, k_star, block, clear, blocked = first_round(H, T, angles)
    resolution, done = delta, 1
    if status == FOUND:
        blocked, clear, block, resolution, done = refine(setting.heights, T, m, blocked, clear, block, resolution, rounds)
    return record(status, done, k_star, block, clear, blocked, resolution, d, lat, lon, T)


def solve(setting, az_lo, az_step, n_az, reach, fan, K, rounds):
    """-> (HORIZON_DTYPE [n_az], azimuths [n_az], the first fan's angles [K])."""
    _, m = sm.lattice(setting.step, reach)
    angles = vm.fan_angles(fan[0], fan[1], K)
    delta = (np.float64(fan[1]) - np.float64(fan[0])) / np.float64(K - 1)
    H = setting.heights(angles, m)
    az = vm.azimuths(az_lo, az_step, n_az)
    out = np.empty(n_az, dtype=HORIZON_DTYPE)
    for j in range(n_az):
        out[j] = solve_one(setting, az[j], reach, angles, delta, H, rounds)
    return out, az, angles


def assert_same(got, want, tag=""):
    """Every field of every record equal; doubles by their bits, every NaN as one value."""
    sm.assert_same(got, want, tag)
