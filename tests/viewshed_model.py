"""The viewshed rule of include/atmrt.h ("viewshed") restated in numpy over sight_model.Setting (the oracle's coords_at_dist, get_elev
and ray_paths of the deterministic flavour).  Test infrastructure only: what atmrt_viewshed must write, plane for plane.  Every
formula below is written as the header states it, one IEEE operation at a time."""
import numpy as np

import sight_model as sm

SEEN, HIDDEN, ABOVE_FAN, BELOW_FAN = sm.SEEN, sm.HIDDEN, sm.ABOVE_FAN, sm.BELOW_FAN
PLANES = (("k_star", np.uint16), ("status", np.uint8), ("hidden", np.float64), ("block_index", np.int32), ("ground", np.float64),
          ("lat", np.float64), ("lon", np.float64))
ONE = np.float64(1.0)
# The ducting setting of the tests on scene S2, whose observer stands at 754 m: atmospheres.inversion(at, thick, gradient) — +5 K/m
# over 20 m, far beyond the +0.12 K/m or so at which a layer starts to duct — with the observer inside the layer at `altitude`
# (Absolute), and a fan narrow enough that many of its rays are trapped: within 12 km rays cross the rays below them.
DUCT = dict(at=744.0, thick=20.0, gradient=5.0, altitude=754.0, fan=(-1.0, 2.0))


def gpu_fan_rays(rays_per_lane):
    """The fans the GPU tests run, from rays_per_lane(K) of the build under test: 64, 128, the smallest K of every variant of the scan
    kernel (every distinct number of rays per lane) and the largest fan, 4096."""
    first = {}
    for K in range(64, 4097, 64):
        first.setdefault(rays_per_lane(K), K)
    return sorted({64, 128, 4096} | set(first.values()))


def fan_angles(lo, hi, K):
    """e_k = lo + (double)k * delta, delta = (hi - lo) / (double)(K - 1)."""
    lo, hi = np.float64(lo), np.float64(hi)
    return lo + np.arange(K, dtype=np.float64) * ((hi - lo) / np.float64(K - 1))


def azimuths(az_lo, az_step, n_az):
    """az_j = az_lo + (double)j * az_step."""
    return np.float64(az_lo) + np.arange(n_az, dtype=np.float64) * np.float64(az_step)


def blocked_at(H, T):
    """H [K][m + 1] against the profile T [m + 1] -> for every ray the first i' >= 1 with c_{i'-1} * c_{i'} < 0.0 or H_{i'-1} < -1000;
    m + 1 where there is none (no cell asks about an i' that large)."""
    with np.errstate(invalid="ignore", over="ignore"):
        c = H - T[None, :]
        stop = (c[:, :-1] * c[:, 1:] < 0.0) | (H[:, :-1] < -1000.0)  # entry i' - 1
    return np.where(stop.any(axis=1), np.argmax(stop, axis=1) + 1, H.shape[1])


def scan(H, T, height):
    """One azimuth: the rays H [K][m + 1] against its profile T [m + 1] -> k_star, status, hidden, block_index, ground, each [m]
    (cell i at i - 1)."""
    K, m = H.shape[0], H.shape[1] - 1
    block = blocked_at(H, T)
    i = np.arange(1, m + 1)
    with np.errstate(invalid="ignore", over="ignore"):
        arrival = H[:, :-1] + ONE * (H[:, 1:] - H[:, :-1])  # [K][m]
        ground = T[:-1] + ONE * (T[1:] - T[:-1])
        aim = ground + np.float64(height)
        fails = (block[:, None] <= i[None, :] - 1) | ~(arrival >= aim[None, :])
    k_star = np.where(fails.any(axis=0), K - np.argmax(fails[::-1], axis=0), 0)
    below = np.maximum(k_star - 1, 0)
    hid = (k_star > 0) & (k_star < K) & (block[below] <= i - 1)
    status = np.where(k_star == K, ABOVE_FAN, np.where(k_star == 0, BELOW_FAN, np.where(hid, HIDDEN, SEEN)))
    at = np.minimum(k_star, K - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        hidden = np.where(k_star == K, np.nan, arrival[at, i - 1] - aim)
    return dict(k_star=k_star.astype(np.uint16), status=status.astype(np.uint8), hidden=hidden, block_index=np.where(hid, block[below], -1).astype(np.int32),
                ground=ground)


def solve(setting, az_lo, az_step, n_az, reach, height, fan, K):
    """-> the planes [n_az][m] by name, plus d [m + 1], azimuths [n_az] and angles [K]."""
    d, m = sm.lattice(setting.step, reach)
    angles = fan_angles(fan[0], fan[1], K)
    H = setting.heights(angles, m)
    az = azimuths(az_lo, az_step, n_az)
    out = {k: np.empty((n_az, m), dtype=t) for k, t in PLANES}
    for j in range(n_az):
        _, mj, lat, lon, T = setting.profile(az[j], reach)
        assert mj == m
        for k, v in scan(H, T, height).items():
            out[k][j] = v
        out["lat"][j], out["lon"][j] = lat[1:], lon[1:]
    out.update(d=d, azimuths=az, angles=angles)
    return out


def assert_same(got, want, tag=""):
    """Every plane equal; doubles by their bits, every NaN as one value.  got: a dict of arrays or an object with such attributes."""
    for name, dtype in PLANES:
        g = got[name] if isinstance(got, dict) else getattr(got, name)
        w = want[name]
        assert g is not None and g.dtype == dtype and g.shape == w.shape, (tag, name, None if g is None else (g.dtype, g.shape), w.shape)
        gv, wv = np.ascontiguousarray(g), np.ascontiguousarray(w)
        if dtype == np.float64:
            gb, wb = gv.view(np.uint64).copy(), wv.view(np.uint64).copy()
            gb[np.isnan(gv)] = wb[np.isnan(wv)] = 0
            gv, wv = gb, wb
        bad = np.argwhere(gv != wv)
        assert bad.size == 0, f"{tag} {name}: {len(bad)} of {gv.size} differ, first at {bad[:5].tolist()}: {g[tuple(bad[:5].T)]} vs {w[tuple(bad[:5].T)]}"
