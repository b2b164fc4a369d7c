"""The host half of the apparent elevation (include/atmrt.h, "apparent elevation"): names and the struct's size, the two host
functions — atmrt_sky_tail_host and atmrt_sky_apparent_host, the function the kernels run — against tests/sky_apparent_model.py bit
for bit over the hand-made tables and over a table filled from atmrt_sky_ray_host, and every refusal that needs no device.  The
library loads without a GPU; nothing here touches a device.  The refusals that need a context are in tests/test_gpu_sky_apparent.py."""
import ctypes as C
import math
import os
import re
import struct

import numpy as np
import pytest

import sky_apparent_cases as sac
import sky_apparent_model as sam
from atm_raytracer_amd import _abi, _lib, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_sky_table", "atmrt_sky_tail_host", "atmrt_sky_apparent_host", "atmrt_sky_apparent", "atmrt_shadow_lights_true_device",
         "atmrt_shadow_lights_true", "atmrt_shadow_lights_true_planes_device", "atmrt_last_sky_table_work")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def same(a, b):
    return struct.pack("d", a) == struct.pack("d", b) or (math.isnan(a) and math.isnan(b))


def test_names_and_struct_size(lib):
    header = open(os.path.join(ROOT, "include", "atmrt.h")).read()
    declared = set(re.findall(r"\b(atmrt_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.atmrt_abi_sizeof(47) == C.sizeof(_abi.SkyTableSpec) == 72
    assert lib.atmrt_abi_sizeof(46) == 0 and lib.atmrt_abi_sizeof(48) == 0
    S = _abi.SkyTableSpec
    assert (S.sky.offset, S.alt_lo.offset, S.alt_hi.offset, S.el_lo.offset, S.el_hi.offset, S.n_alt.offset, S.n_el.offset) == (0, 32, 40, 48, 56, 64, 68)
    assert lib.atmrt_abi_version() == 5  # the additions are additive
    assert "apparent elevation" in header and "TRUE-DIRECTION SHADOW LIGHTS" in header and "LIMITATION" in header


def test_hand_made_tables_equal_the_model_bit_for_bit(lib):
    spec = sac.abi_spec(sac.hand_spec())
    # the tail rule, three rows at a time (the spec's n_alt)
    rows = sac.TAIL_ROWS
    for at in range(0, len(rows), 3):
        T = np.array([r[0] for r in rows[at:at + 3]])
        S = np.array([r[1] for r in rows[at:at + 3]], dtype=np.uint8)
        got = generators.sky_tail_host(spec, T, S, lib)
        assert got.tolist() == [r[2] for r in rows[at:at + 3]] == sam.tails(T, S).tolist(), (at, got)
    table = sac.hand_table()
    for h, t, want in sac.APPARENT_ANSWERS:
        got = generators.sky_apparent_host(spec, table.T, table.tail, h, t, lib)
        assert same(got, want) and same(got, sam.apparent(table, h, t)), (h, t, got, want)
    # every row answer through a level of its own: h on level j gives row j (f = 0) for j < n_alt - 1, level 2 gives row 2 (f = 1)
    for j, t, want, _ in sac.ROW_ANSWERS:
        got = generators.sky_apparent_host(spec, table.T, table.tail, table.spec.alt(j), t, lib)
        assert same(got, want), (j, t, got, want)
    # the last usable tail, n_el - 2, in every row
    T3, _, tail3 = sac.TAIL_ROWS[3]
    for t, want, _ in sac.LAST_TAIL_ANSWERS:
        assert same(generators.sky_apparent_host(spec, np.array([T3] * 3), [tail3] * 3, 123.0, t, lib), want), t


def test_a_marched_table_equals_the_model_bit_for_bit(lib):
    """US-76 on the sphere, 3 x 257 entries from -3 degrees at 0.05 degrees, filled from atmrt_sky_ray_host (which
    tests/test_sky_abi.py pins to the model): the tails, then apparent(h, t) over a list that reaches every arm, asserted by a census."""
    cfg, top = sac.setting_of("us76_sphere")
    mspec = sac.table_spec(3, 257, top)
    spec = sac.abi_spec(mspec)
    T, S = np.full((3, 257), np.nan), np.zeros((3, 257), dtype=np.uint8)
    for j in range(3):
        for k in range(257):
            S[j, k], _, T[j, k] = generators.sky_ray_host(cfg.atmosphere, cfg.params.wavelength, cfg.params.earth, False, spec.sky, mspec.alt(j),
                                                          mspec.el(k), lib)
    table = sam.Table(mspec, T, S)
    tail = generators.sky_tail_host(spec, T, S, lib)
    assert tail.tobytes() == table.tail.tobytes() and table.usable.all() and (table.tail > 0).all()
    h, t = sac.census_pairs(table)
    census = {}
    for a, b in zip(h, t):
        got = generators.sky_apparent_host(spec, T, tail, a, b, lib)
        want, j, f, arm_a, arm_b = sam.apparent_parts(table, a, b)
        assert same(got, want), (a, b, got, want)
        for arm in (arm_a, arm_b):
            census[arm] = census.get(arm, 0) + 1
        if j is not None:
            clamp = "clamped low" if a < mspec.alt_lo else ("clamped high" if a > mspec.alt_hi else "in range")
            census[clamp] = census.get(clamp, 0) + 1
    print(f"apparent host census: {census}")
    assert all(census.get(k, 0) > 0 for k in ("inside", "below", "above", "nan", None, "clamped low", "clamped high", "in range"))


def test_refusals(lib):
    bad, nan, inf = _abi.ERR_INVALID_ARGUMENT, math.nan, math.inf
    table = sac.hand_table()
    good = sac.abi_spec(table.spec)
    T, S = np.ascontiguousarray(table.T), np.ascontiguousarray(table.S)
    tail = np.full(3, 77, dtype=np.uint32)
    out = C.c_double(77.0)
    ok_tail = np.ascontiguousarray(table.tail)

    def tails(spec=good, t=T.ctypes.data, s=S.ctypes.data, o=tail.ctypes.data):
        return lib.atmrt_sky_tail_host(None if spec is None else C.byref(spec), t, s, o)

    def inverse(spec=good, t=T.ctypes.data, tl=ok_tail.ctypes.data, o=C.byref(out)):
        return lib.atmrt_sky_apparent_host(None if spec is None else C.byref(spec), t, tl, 250.0, 1.25, o)

    assert inverse() == 0 and out.value == 1.625
    out.value = 77.0
    assert tails(spec=None) == bad and tails(t=None) == bad and tails(s=None) == bad and tails(o=None) == bad
    assert inverse(spec=None) == bad and inverse(t=None) == bad and inverse(tl=None) == bad and inverse(o=None) == bad

    def spec_of(alt=sac.HAND_ALT, el=sac.HAND_EL, **sky):
        sky = dict(dict(step=1000.0, top=100000.0, floor=0.0, m=1500), **sky)
        return generators.sky_table_spec(alt, el, **sky)

    refused = [spec_of(alt=(0.0, 0.0, 3)), spec_of(alt=(1000.0, 0.0, 3)), spec_of(alt=(nan, 1000.0, 3)), spec_of(alt=(0.0, inf, 3)),
               spec_of(alt=(-inf, 0.0, 3)), spec_of(el=(-90.0, 4.0, 5)), spec_of(el=(0.0, 90.0, 5)), spec_of(el=(4.0, 4.0, 5)),
               spec_of(el=(4.0, 0.0, 5)), spec_of(el=(nan, 4.0, 5)), spec_of(el=(0.0, nan, 5)), spec_of(el=(-inf, 4.0, 5)),
               spec_of(alt=(0.0, 1000.0, 1)), spec_of(alt=(0.0, 1000.0, 0)), spec_of(alt=(0.0, 1000.0, 1025)), spec_of(el=(0.0, 4.0, 1)),
               spec_of(el=(0.0, 4.0, 0)), spec_of(el=(0.0, 4.0, 65537)), spec_of(alt=(0.0, 1000.0, 257), el=(0.0, 4.0, 65536)),
               spec_of(step=-1.0), spec_of(step=nan), spec_of(top=nan), spec_of(floor=inf), spec_of(top=0.0, floor=0.0), spec_of(m=0),
               spec_of(m=1048576)]
    for k, spec in enumerate(refused):
        assert tails(spec=spec) == bad and inverse(spec=spec) == bad, k
    assert (tail == 77).all() and out.value == 77.0
    # a table with a row that is not usable: the inverse refuses it, whichever row it is; the tail rule does not
    for j in range(3):
        for t in (4, 5, 6, 0xffffffff):
            unusable = ok_tail.copy()
            unusable[j] = t
            assert inverse(tl=unusable.ctypes.data) == bad, (j, t)
        last = ok_tail.copy()
        last[j] = 3  # n_el - 2: usable
        assert inverse(tl=last.ctypes.data) == 0
    out.value = 77.0
    assert tails(spec=spec_of(step=0.0)) == 0 and tail.tolist() == sac.HAND_TAIL  # step 0 (the context's) is a valid spec
    # the entry points refuse a NULL context before they look at anything else
    buf = np.zeros(64, dtype=np.uint64)
    p = buf.ctypes.data
    lights, keep = generators.shadow_lights_spec([[1.0, 0.0, 0.2]], 1e4)
    assert lib.atmrt_sky_table(None, C.byref(good), p, p, p, None) == bad
    assert lib.atmrt_sky_apparent(None, C.byref(good), 4, p, p, p) == bad
    assert lib.atmrt_shadow_lights_true(None, C.byref(lights), C.byref(good), p, None, None, None) == bad
    assert lib.atmrt_shadow_lights_true_device(None, C.byref(lights), C.byref(good), p, None, None, None) == bad
    assert lib.atmrt_shadow_lights_true_planes_device(None, C.byref(lights), C.byref(good), 8, p, p, p, p, p, None, None, None) == bad
    assert lib.atmrt_last_sky_table_work(None, C.byref(C.c_int32()), (C.c_double * 3)()) == bad
    assert not buf.any()
