"""The host half of the viewshed map (include/atmrt.h): the three entry points' names, the stats struct against the header, and NULL
arguments.  The library loads without a GPU; nothing here touches a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import viewshed_map_model as mm
from atm_raytracer_amd import _abi, _lib, generators

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("atmrt_viewshed_map_planes_device", "atmrt_viewshed_map_device", "atmrt_viewshed_map")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.load()


def test_names_and_struct_layout(lib):
    header = open(os.path.join(ROOT, "include", "atmrt.h")).read()
    declared = set(re.findall(r"\b(atmrt_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in declared and name in _lib.EXPORTED and hasattr(lib, name), name
    assert lib.atmrt_abi_sizeof(33) == C.sizeof(_abi.ViewshedMapStats) == 40
    assert lib.atmrt_abi_sizeof(32) == 0 and lib.atmrt_abi_sizeof(34) == 0 and lib.atmrt_abi_version() == 5
    # the struct of the header, field for field: five u64 in the header's order
    body = re.search(r"typedef struct atmrt_viewshed_map_stats \{(.*?)\} atmrt_viewshed_map_stats_t;", header, re.S).group(1)
    fields = [f.strip() for decl in re.findall(r"uint64_t ([^;]+);", body) for f in decl.split(",")]
    assert fields == [n for n, _ in _abi.ViewshedMapStats._fields_] == list(mm.STATS)
    assert [getattr(_abi.ViewshedMapStats, n).offset for n in fields] == [0, 8, 16, 24, 32]
    assert all(t is C.c_uint64 for _, t in _abi.ViewshedMapStats._fields_)
    assert lib.atmrt_abi_sizeof(18) == C.sizeof(_abi.GeoGrid) == 40 and lib.atmrt_abi_sizeof(28) == C.sizeof(_abi.ViewshedSpec) == 56
    assert "viewshed map" in header and "n_samples = n_binned + n_outside + n_skipped" in header
    assert [k for k, _ in generators.VIEWSHED_MAP_PLANES] == [k for k, _ in mm.PLANES]
    assert [np.dtype(t) for _, t in generators.VIEWSHED_MAP_PLANES] == [np.dtype(t) for _, t in mm.PLANES]


def test_null_arguments(lib):
    """A NULL context: refused with nothing to write the message to.  No context can be made without a device, so the other NULL
    arguments are tested on the GPU (tests/test_gpu_viewshed_map.py)."""
    spec = _abi.ViewshedSpec(0.0, 1.0, 1_000.0, 0.0, -1.0, 1.0, 1, 64)
    grid = _abi.GeoGrid(0.0, 0.0, 1.0, 1.0, 2, 2)
    ns, nv, mh = np.full(4, 7, np.uint32), np.full(4, 7, np.uint32), np.full(4, 7.0)
    st = _abi.ViewshedMapStats(9, 9, 9, 9, 9)
    status, f = np.zeros(4, np.uint8), np.zeros(4)
    for fn in (lib.atmrt_viewshed_map, lib.atmrt_viewshed_map_device):
        assert fn(None, C.byref(spec), C.byref(grid), 0, ns.ctypes.data, nv.ctypes.data, mh.ctypes.data, C.byref(st)) == _abi.ERR_INVALID_ARGUMENT
        assert fn(None, None, None, 0, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_viewshed_map_planes_device(None, C.byref(grid), 4, status.ctypes.data, f.ctypes.data, f.ctypes.data, f.ctypes.data, 0, ns.ctypes.data,
                                                nv.ctypes.data, mh.ctypes.data, C.byref(st)) == _abi.ERR_INVALID_ARGUMENT
    assert lib.atmrt_viewshed_map_planes_device(None, None, 0, None, None, None, None, 0, None, None, None, None) == _abi.ERR_INVALID_ARGUMENT
    assert (ns == 7).all() and (nv == 7).all() and (mh == 7.0).all() and st.n_samples == 9 and st.n_seen == 9  # a refused call writes nothing
