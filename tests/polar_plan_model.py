"""How the calls along azimuths from the observer (sight lines, viewshed, viewshed map, horizon) split their targets into batches, and how
many samples a reach takes — restated in Python from the host code as it stood before the calls shared one planner (sight_plan,
viewshed_run and horizon_run of csrc/atmrt_api.hip), not from csrc/atmrt_polar_plan.h.  tests/test_polar_plan_host.py holds the
planner to it on the CPU; the test_batches* tests on the GPU take the batch count they expect from it.

A plan is (batch_begin, entries_max, off): the first target of every batch and n at the end, the profile entries of the largest
batch, and per target the first entry of its profile counted from the start of its batch."""

SIGHT_TARGET, SIGHT_META, DIR_CALC, HORIZON_RECORD = 24, 16, 128, 72  # bytes of atmrt_sight_target_t, SightMeta, DirCalc, atmrt_horizon_t
SCRATCH_BYTES = 200 << 20
M_MAX = 65535


def pad(n):
    """Carve: every array of a batch begins on a multiple of 256 bytes"""
    return (n + 255) // 256 * 256


def steps(step, reach, m_max=M_MAX):
    """The first index i with d_i >= reach, d_0 = 0 and d_{i+1} = d_i + step; None where that is more than m_max samples away."""
    d, i = 0.0, 0
    while d < reach:
        d += step
        i += 1
        if i > m_max:
            return None
    return i


def target_bytes(m):
    """what a target's profile adds to a batch: three doubles per sample and a kilobyte"""
    return 3 * 8 * (m + 1) + 1024


def greedy(ms, limit, extra=0):
    """sight_plan: targets in order, a new batch where the next target would pass the limit; a batch holds at least one"""
    begin, off, nbytes, entries, entries_max = [0], [], 0, 0, 0
    for t, m in enumerate(ms):
        add = target_bytes(m) + extra
        if nbytes and nbytes + add > limit:
            begin.append(t)
            nbytes = entries = 0
        off.append(entries)
        nbytes += add
        entries += m + 1
        entries_max = max(entries_max, entries)
    return begin + [len(ms)], entries_max, off


def layout_bytes(nb, m, staged):
    """sight_carve over a null base for nb targets of m samples, and the call's arrays of staged[j] bytes per target beside them"""
    n = pad(8 * (m + 1)) + pad(8) + pad(SIGHT_TARGET * nb) + pad(SIGHT_META * nb) + pad(DIR_CALC * nb) + 3 * pad(8 * nb * (m + 1))
    return n + sum(pad(nb * s) for s in staged)


def uniform(n, m, limit, staged):
    """viewshed_run / horizon_run: min(n, max(1, limit / per_az)) azimuths to a batch, then one fewer while the whole layout passes the limit"""
    per_az = target_bytes(m) + sum(staged)
    nb = min(n, max(1, limit // per_az))
    while nb > 1 and layout_bytes(nb, m, staged) > limit:
        nb -= 1
    return list(range(0, n, nb)) + [n], nb * (m + 1), [(t % nb) * (m + 1) for t in range(n)]


def viewshed_staged(m, block_index=True, ground=True, lat=True, lon=True):
    """the planes atmrt_viewshed stages per azimuth on its host route: k_star, status and hidden always, the rest where asked"""
    return [2 * m, m, 8 * m] + [4 * m] * block_index + [8 * m] * ground + [8 * m] * lat + [8 * m] * lon


def viewshed_map_staged(m):
    """the planes a fused map call stages per azimuth: status, hidden, lat, lon (25 bytes per cell)"""
    return [m, 8 * m, 8 * m, 8 * m]


HORIZON_STAGED = [HORIZON_RECORD]  # atmrt_horizon's host route; both device routes stage nothing: []


def batches(plan):
    return len(plan[0]) - 1
