"""The route of the first-pass Rectilinear march and the layout of the time-sliced march's state, restated from the rule the march
plan (csrc/atmrt_march_plan.h) has to keep — the table of routes by override and mode, not the header's code.
tests/test_march_plan_host.py compares the header with it case by case."""

NONE, PLAIN, SMALL, SLICED, QUEUE = range(5)           # ATMRT_MARCH_VARIANT: unset, plain, small, sliced, queue
R_NONE, R_GRID, R_DRAIN, R_SLICED, R_QUEUE = range(5)  # MarchRoute
SMALL_MAX_BLOCKS = 16384
DRAIN_MAX_BLOCKS = {0: 16384, 1: 6144, 2: 16384, 3: 12288}  # by k_rect_march's MODE
SLICE_STEPS = 128
GROUP_LIST_BYTES = 96 * (4 * 8 + 4) + 2 * 8  # a group's candidate list: 96 entries of four doubles and an index, two doubles in front


def ceil_div(a, b):
    return -(-a // b)


def blocks(n):
    return ceil_div(n, 256)


def can_slice(n, n_t):
    return n > 0 and n_t + 2 > SLICE_STEPS and ceil_div(n, 64) * ceil_div(n_t + 2, SLICE_STEPS) <= 0x7FFFFFFF


def grid(mode, n, override):
    """mode 2, the fall-back of a queue that cannot be launched, and every launch the rows below leave to its size"""
    if override == PLAIN:
        return R_GRID
    if override in (SMALL, SLICED):
        return R_DRAIN
    return R_DRAIN if blocks(n) <= DRAIN_MAX_BLOCKS[mode] else R_GRID


def _by_size(n, n_t, mode, queue_ok):  # the row "none"
    if mode == 0:
        if blocks(n) <= SMALL_MAX_BLOCKS:
            return R_SLICED if can_slice(n, n_t) else R_DRAIN
        return R_QUEUE if queue_ok else R_GRID
    return R_DRAIN if blocks(n) <= DRAIN_MAX_BLOCKS[mode] else R_GRID


def route(n, n_t, mode, queue_ok, override):
    assert mode in (0, 1, 3)
    if override == PLAIN:
        return R_GRID
    if override == SMALL:
        return R_DRAIN
    if override == SLICED:
        return R_SLICED if can_slice(n, n_t) else R_DRAIN
    if override == QUEUE and mode == 0 and queue_ok:
        return R_QUEUE
    return _by_size(n, n_t, mode, queue_ok)


def pad256(n):
    return ceil_div(n, 256) * 256


def slices(n, n_t, objects):
    """n_groups, n_pad, slices_after, cap, bytes of a sliced launch"""
    n_groups = ceil_div(n, 64)
    n_pad = 64 * n_groups
    after = ceil_div(n_t + 2, SLICE_STEPS)
    cap = n_groups * after
    nbytes = n_pad * 196 + 64 + 4 * cap
    if objects:
        nbytes = pad256(nbytes) + n_groups * GROUP_LIST_BYTES
    return n_groups, n_pad, after, cap, nbytes


ARRAYS = ("calc", "x", "a", "b", "sh", "pl", "diff0", "ang", "step", "hint", "count", "ctl", "queue", "glist")
ELEMENT = dict(calc=(128, 8), x=(8, 8), a=(8, 8), b=(8, 8), sh=(8, 8), pl=(8, 8), diff0=(8, 8), ang=(8, 8), step=(4, 4), hint=(4, 4),
               count=(4, 4), ctl=(8, 8), queue=(4, 4), glist=(1, 8))  # bytes and alignment of an element (a list begins with doubles)


def layout(n, n_t, objects):
    """{array: (offset, bytes)} of the block, in its order; glist only with objects"""
    n_groups, n_pad, _, cap, _ = slices(n, n_t, objects)
    out, off = {}, 0
    for name in ARRAYS[:11]:
        out[name] = (off, n_pad * ELEMENT[name][0])
        off += n_pad * ELEMENT[name][0]
    out["ctl"] = (off, 64)
    out["queue"] = (off + 64, 4 * cap)
    if objects:
        out["glist"] = (pad256(off + 64 + 4 * cap), n_groups * GROUP_LIST_BYTES)
    return out
