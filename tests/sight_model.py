"""The sight-line rule of include/atmrt.h ("sight lines") restated in numpy over the oracle's primitives: coords_at_dist, get_elev
and ray_paths of the deterministic flavour.  Test infrastructure only: what atmrt_sight_lines / atmrt_sight_fan_probe must return,
field for field.  Every formula below is written as the header states it, one IEEE operation at a time."""
import numpy as np

from atm_raytracer_amd import _abi

SEEN, HIDDEN, ABOVE_FAN, BELOW_FAN = 0, 1, 2, 3
M_MAX = 65535

SIGHT_DTYPE = np.dtype([("status", np.int32), ("rounds_done", np.int32), ("m", np.int32), ("block_index", np.int32)] +
                       [(k, np.float64) for k in ("angle", "arrival", "ground", "hidden", "resolution", "block_distance", "block_lat",
                                                  "block_lon", "block_elevation")])
RAY_DTYPE = np.dtype([("block_index", np.int32), ("min_index", np.int32), ("arrival", np.float64), ("min_clearance", np.float64)])


def fan_angles(lo, hi):
    """e_k = lo + (double)k * delta, delta = (hi - lo) / 63.0."""
    lo, hi = np.float64(lo), np.float64(hi)
    return lo + np.arange(64, dtype=np.float64) * ((hi - lo) / np.float64(63.0))


def pick(fails):
    """k*: one above the highest failing ray; 0 if none fails."""
    idx = np.flatnonzero(np.asarray(fails).astype(bool))
    return int(idx[-1]) + 1 if idx.size else 0


def lattice(step, distance):
    """d_0 = 0, d_i = d_{i-1} + step as far as the first d_m >= distance -> (d [m + 1], m)."""
    d, x = [0.0], 0.0
    while not x >= distance:
        x = x + step
        d.append(x)
        if len(d) - 1 > M_MAX:
            raise ValueError("more than 65535 samples")
    return np.array(d, dtype=np.float64), len(d) - 1


class Setting:
    """The context's setting on the oracle's side: parameters, atmosphere and terrain tiles."""

    def __init__(self, oracle, cfg, tiles):
        self.o, self.params, self.atm = oracle, cfg.params, cfg.atmosphere
        self.terrain = oracle.terrain_new(tiles)
        pos = self.params.position
        self.alt = pos.altitude if pos.altitude_kind == _abi.ALT_ABSOLUTE else self.elev(pos.latitude, pos.longitude) + pos.altitude
        self.step = self.params.simulation_step
        self._profiles, self._paths = {}, {}

    def close(self):
        self.o.terrain_free(self.terrain)

    def elev(self, lat, lon):
        e = self.o.get_elev(self.terrain, lat, lon)
        return 0.0 if e is None else e

    def profile(self, azimuth_deg, distance):
        """-> (d, m, lat, lon, T) of the target's sample lattice."""
        key = (float(azimuth_deg), float(distance))
        if key not in self._profiles:
            d, m = lattice(self.step, distance)
            pos = self.params.position
            ll = self.o.coords_at_dist(self.params.earth, pos.latitude, pos.longitude, azimuth_deg, d)
            T = np.array([self.elev(a, b) for a, b in ll], dtype=np.float64)
            self._profiles[key] = (d, m, ll[:, 0].copy(), ll[:, 1].copy(), T)
        return self._profiles[key]

    def heights(self, angles_deg, m):
        """H [n][m + 1]: H_0 = alt, H_i = the stepper's h after i steps."""
        ang = np.ascontiguousarray(angles_deg, dtype=np.float64)
        _, h = self.o.ray_paths(self.params, self.alt, ang, self.step, m, straight=bool(self.params.straight_rays), atm=self.atm)
        return h


def trace(H, T, d, m, distance):
    """The rays of H [n][m + 1] against the profile -> RAY_DTYPE [n]."""
    n = H.shape[0]
    out = np.empty(n, dtype=RAY_DTYPE)
    prop = (np.float64(distance) - d[m - 1]) / (d[m] - d[m - 1])
    with np.errstate(invalid="ignore", over="ignore"):
        c = H[:, :m] - T[None, :m]  # c_i, i <= m - 1
        stop = (c[:, :-1] * c[:, 1:] < 0.0) | (H[:, :m - 1] < -1000.0)  # entry i - 1: blocked at i, 1 <= i <= m - 1
        arrival = H[:, m - 1] + prop * (H[:, m] - H[:, m - 1])
    for k in range(n):
        at = np.flatnonzero(stop[k])
        block = int(at[0]) + 1 if at.size else -1
        last = block if block >= 0 else m - 1
        best, where = c[k, 0], 0  # a later c_i replaces it only when it is smaller: the first minimum; nothing is smaller than a NaN
        if not np.isnan(best):
            seg = np.where(np.isnan(c[k, :last + 1]), np.inf, c[k, :last + 1])
            where = int(np.argmin(seg))
            best = seg[where]
        out[k] = (block, where, np.nan if block >= 0 or np.isnan(arrival[k]) else arrival[k], best)
    return out


def fan_probe(setting, target, angles_deg):
    az, distance, _ = target
    d, m, _, _, T = setting.profile(az, distance)
    return trace(setting.heights(angles_deg, m), T, d, m, distance)


def solve_one(setting, target, lo, hi, rounds):
    az, distance, height = (np.float64(v) for v in target)
    d, m, lat, lon, T = setting.profile(az, distance)
    prop = (distance - d[m - 1]) / (d[m] - d[m - 1])
    ground = T[m - 1] + prop * (T[m] - T[m - 1])
    aim = ground + height
    lo, hi = np.float64(lo), np.float64(hi)
    for r in range(rounds):
        e = fan_angles(lo, hi)
        delta = (hi - lo) / np.float64(63.0)
        rays = trace(setting.heights(e, m), T, d, m, distance)
        with np.errstate(invalid="ignore"):
            fails = (rays["block_index"] >= 0) | ~(rays["arrival"] >= aim)
        k = pick(fails)
        done = r + 1
        if k in (0, 64) or done == rounds:
            break
        lo, hi = e[k - 1], e[k]
    rec = np.zeros((), dtype=SIGHT_DTYPE)
    rec["rounds_done"], rec["m"], rec["ground"], rec["resolution"] = done, m, ground, delta
    below = rays[k - 1] if k > 0 else None
    rec["status"] = ABOVE_FAN if k == 64 else BELOW_FAN if k == 0 else HIDDEN if below["block_index"] >= 0 else SEEN
    if k == 64:
        rec["angle"] = rec["arrival"] = rec["hidden"] = np.nan
    else:
        rec["angle"], rec["arrival"] = e[k], rays["arrival"][k]
        with np.errstate(invalid="ignore"):
            hidden = rays["arrival"][k] - aim
        rec["hidden"] = np.nan if np.isnan(hidden) else hidden
    if rec["status"] == HIDDEN:
        i = int(below["block_index"])
        rec["block_index"], rec["block_distance"], rec["block_lat"], rec["block_lon"], rec["block_elevation"] = i, d[i], lat[i], lon[i], T[i]
    else:
        rec["block_index"] = -1
        rec["block_distance"] = rec["block_lat"] = rec["block_lon"] = rec["block_elevation"] = np.nan
    return rec


def solve(setting, targets, fan=(-5.0, 5.0), rounds=3):
    """targets: rows of (azimuth_deg, distance, height) -> SIGHT_DTYPE [n].  Equal targets are solved once."""
    out = np.empty(len(targets), dtype=SIGHT_DTYPE)
    seen = {}
    for i, t in enumerate(targets):
        key = tuple(float(v) for v in t)
        if key not in seen:
            seen[key] = solve_one(setting, key, fan[0], fan[1], rounds)
        out[i] = seen[key]
    return out


def assert_same(got, want, tag=""):
    """Every field of every record equal; doubles by their bits, every NaN as one value."""
    assert got.dtype == want.dtype and got.shape == want.shape, (tag, got.dtype, want.dtype, got.shape, want.shape)
    for name in got.dtype.names:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        if g.dtype == np.float64:
            gb, wb = g.view(np.uint64).copy(), w.view(np.uint64).copy()
            gb[np.isnan(g)] = wb[np.isnan(w)] = 0
            g, w = gb, wb
        bad = np.flatnonzero(g != w)
        assert bad.size == 0, f"{tag} {name}: {bad.size} of {g.size} differ, first at {bad[:5]}: {got[name][bad[:5]]} vs {want[name][bad[:5]]}"
