"""A numpy restatement of what the Rectilinear lean march does with the terrain ceiling table — the rule of march_steps
(csrc/atmrt_march_impl.h), not the oracle's, which has no table:

    diff0 = h[0] - terrain(sample 0)
    for i = 1, 2, ... while xs[i] <= max_distance and h[i] >= -1000:
        entry = table[min(i, rows - 1)][bin]              # the ray's bin, from its direction and the layout's three doubles
        diff1 = h[i] > entry.cell ? (any positive number) : h[i] - terrain(sample i)
        if diff0 * diff1 < 0: the first crossing is in step i - 1; opaque terrain ends the ray
        if h[i] > max(entry.suffix, escape floor) and the ray is ascending: the ray leaves, a miss
        diff0 = diff1

Everything the rule consumes comes from the oracle (det flavour): the rays' heights from ray_paths at the pixel's elevation angle,
the sample positions from coords_at_dist at the pixel's azimuth, the terrain from get_elev; azimuth and elevation angle are the
planes of the oracle's own frame.  "Ascending" is restated as h[i] > h[i - 1]: the kernel tests the stepper's dr/dphi, which has
that sign for a refracted ray above the certificate's floor.  With the right table the two shortcuts change nothing (that is
their claim, and tests/test_ceiling_teeth.py checks it against the oracle's frame); with a table whose rows or bins are shifted
the model says which pixels a march with that index slip would get wrong."""
import math

import numpy as np

from atm_raytracer_amd import _abi


def bins_of(layout, n_bins, azimuth_deg):
    """ceiling_bin (csrc/atmrt_ceiling.h) of directions given in degrees; n_bins for a direction outside the bins"""
    dir0, rel_lo, w = layout
    rel = np.radians(azimuth_deg) - dir0
    rel = rel - 2.0 * math.pi * np.floor((rel + math.pi) / (2.0 * math.pi))
    t = (rel - rel_lo) * (1.0 / w)
    inside = (t >= 0.0) & (t < n_bins)
    return np.where(inside, np.where(inside, t, 0.0).astype(np.int64), n_bins)


class Frame:
    """The inputs of the rule for the pixels `columns` (all rows) of the opaque frame `cfg` over `tiles`; `want` is the oracle's
    own frame of cfg."""

    def __init__(self, oracle, cfg, tiles, want, columns, altitude):
        p = cfg.params
        self.columns = np.asarray(columns)
        self.az = want["azimuth"][:, self.columns].ravel()
        self.el = want["elevation_angle"][:, self.columns].ravel()
        step, reach = p.simulation_step, p.frame.max_distance
        xs = [0.0]
        while xs[-1] + step <= reach:
            xs.append(xs[-1] + step)  # the distance table: repeated addition
        self.xs = np.array(xs)
        n = len(xs) - 1
        x, self.h = oracle.ray_paths(p, altitude, self.el, step, n, bool(p.straight_rays), cfg.atmosphere)
        assert np.array_equal(x[0], self.xs)
        earth = _abi.EarthModel()
        earth.kind, earth.radius = p.earth.kind, p.earth.radius
        t = oracle.terrain_new(tiles)
        try:
            self.ground = np.empty_like(self.h)
            for k, az in enumerate(self.az):
                for i, (lat, lon) in enumerate(oracle.coords_at_dist(earth, p.position.latitude, p.position.longitude, float(az), self.xs)):
                    e = oracle.get_elev(t, lat, lon)
                    self.ground[k, i] = 0.0 if e is None else e
        finally:
            oracle.terrain_free(t)
        # what the oracle saw: hit or miss, and the distance of the first trace point
        count = want["hit_count"][:, self.columns].ravel()
        first = want["hit_offset"][:, self.columns].ravel().astype(np.int64)
        self.want_hit = count > 0
        self.want_distance = np.where(self.want_hit, want["distance"][np.where(self.want_hit, first, 0)], np.nan)

    def march(self, layout, cell, suffix, escape_floor):
        """(first crossing's step or -1, the step at which the ray left or -1, lookups) per modelled pixel"""
        rows, n_bins = cell.shape[0], cell.shape[1] - 1
        bins = bins_of(layout, n_bins, self.az)
        n_px, n = self.h.shape
        first, left = np.full(n_px, -1), np.full(n_px, -1)
        lookups = np.ones(n_px, dtype=np.int64)
        alive = np.ones(n_px, dtype=bool)
        diff0 = self.h[:, 0] - self.ground[:, 0]
        for i in range(1, n):
            row = min(i, rows - 1)
            sh = self.h[:, i]
            alive &= ~(sh < -1000.0)
            above = sh > cell[row, bins]
            lookups += alive & ~above
            diff1 = np.where(above, 1.0, sh - self.ground[:, i])
            crossing = alive & (diff0 * diff1 < 0.0)
            first[crossing] = i - 1
            alive &= ~crossing
            leaves = alive & (sh > np.maximum(suffix[row, bins], escape_floor)) & (sh > self.h[:, i - 1])
            left[leaves] = i
            alive &= ~leaves
            diff0 = diff1
        return first, left, lookups

    def agrees_with_the_oracle(self, first):
        """per pixel: hit/miss as in the oracle's frame and the oracle's first trace point inside the crossing's step"""
        hit = first >= 0
        lo, hi = self.xs[np.maximum(first, 0)], self.xs[np.minimum(np.maximum(first, 0) + 1, len(self.xs) - 1)]
        inside = (self.want_distance >= lo) & (self.want_distance <= hi)
        return (hit == self.want_hit) & (~hit | inside)
