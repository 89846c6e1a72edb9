"""The C ABI of the projected tree reads (sdb_lsm_scan_projected, sdb_lsm_get_projected): the symbols, the sizers
against the filtered calls' over the recorded grid, the host checks of rule P5 and the no-device path.  No device is
needed."""
import ctypes as C
import itertools
import json
import os
import re
import subprocess

import pytest

from slatedb_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("sdb_lsm_scan_projected", "sdb_lsm_scan_projected_workspace_bytes", "sdb_lsm_get_projected",
       "sdb_lsm_get_projected_workspace_bytes")


@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


def test_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "slatedb_amd", "libslatedb_amd.so")]).decode()
    exported = set(re.findall(r" T (sdb_\w+)", out))
    assert set(NEW) <= exported and set(NEW) <= set(_abi.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "slatedb_amd.h")).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
    assert lib.sdb_abi_version() == 2  # no struct changed


def test_sizers_hold_the_filtered_calls(lib):
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "read_workspace_bytes.json")))
    for new, old in (("sdb_lsm_get_projected_workspace_bytes", "sdb_lsm_get_filtered_workspace_bytes"),
                     ("sdb_lsm_scan_projected_workspace_bytes", "sdb_lsm_scan_filtered_workspace_bytes")):
        axes = g["axes"][old]
        points = list(itertools.product(*[g["grid"][a] for a in axes]))
        assert len(points) == len(g["sizes"][old])
        for point, recorded in zip(points, g["sizes"][old]):
            args = [y for x in point for y in (x if isinstance(x, list) else [x])]
            assert getattr(lib, old)(*args) == recorded
            assert getattr(lib, new)(*args) >= recorded, (new, point)


def _ranges(n, p):
    return _abi.ScanRanges(n, p, p, p, p, p, p)


def _without(rg, field):
    vals = {f: getattr(rg, f) for f, _ in _abi.ScanRanges._fields_}
    vals[field] = None
    return _abi.ScanRanges(*[vals[f] for f, _ in _abi.ScanRanges._fields_])


ARRAYS = [f for f, _ in _abi.ScanRanges._fields_ if f != "n"]


def test_scan_projected_host_checks(lib):
    keep = [(C.c_uint64 * 64)() for _ in range(8)]
    p = [C.addressof(k) for k in keep]
    lsm = _abi.LsmView(p[0], 1, 1, p[0], p[0], p[0], p[0], p[0], p[0], 4)
    rg, proj = _ranges(1, p[1]), _ranges(1, p[7])
    out = _abi.LsmScanOut(p[2], p[2], p[2], p[2], 0, p[2], p[2], p[2], p[2], p[2], p[2], p[2], p[2], 0, p[3])
    fout = _abi.ScanFilterOut(p[5], p[6])
    wsb = lib.sdb_lsm_scan_projected_workspace_bytes(4, 1, 1, 1, 0, 0, 0)
    ws = (C.c_uint8 * (wsb + 256))()

    def call(proj_, fout_=fout, n=wsb):
        return lib.sdb_lsm_scan_projected(C.byref(lsm), None if proj_ is None else C.byref(proj_), None, C.byref(rg), None,
                                          None, 0, 0, 0, C.byref(out), None, None if fout_ is None else C.byref(fout_),
                                          ws, n, None)

    assert call(_ranges(2, p[7])) == _abi.SDB_INVALID_ARGUMENT and call(_ranges(0, p[7])) == _abi.SDB_INVALID_ARGUMENT
    for f in ARRAYS:
        assert call(_without(proj, f)) == _abi.SDB_INVALID_ARGUMENT, f  # a NULL array inside proj
    assert call(proj, None) == _abi.SDB_INVALID_ARGUMENT and call(None, None) == _abi.SDB_INVALID_ARGUMENT  # a NULL fout
    assert call(proj, fout, wsb - 1) == _abi.SDB_INVALID_ARGUMENT
    if lib.sdb_device_count() == 0:  # after the host checks, without a device
        assert call(proj) == _abi.SDB_DEVICE_ERROR
        assert call(None) == _abi.SDB_DEVICE_ERROR


def test_get_projected_host_checks(lib):
    keep = [(C.c_uint64 * 64)() for _ in range(5)]
    p = [C.addressof(k) for k in keep]
    lsm = _abi.LsmView(p[0], 1, 1, p[0], p[0], p[0], p[0], p[0], p[0], 4)
    proj = _ranges(1, p[4])
    out = _abi.GetOut(*([p[1]] * 12), p[2])
    wsb = lib.sdb_lsm_get_projected_workspace_bytes(4, 1, 1, 1, 0)
    ws = (C.c_uint8 * (wsb + 256))()

    def call(proj_, out_=out, n=wsb):
        return lib.sdb_lsm_get_projected(C.byref(lsm), None if proj_ is None else C.byref(proj_), None, p[3], p[3], 1, None,
                                         None, None if out_ is None else C.byref(out_), None, ws, n, None)

    assert call(_ranges(2, p[4])) == _abi.SDB_INVALID_ARGUMENT and call(_ranges(0, p[4])) == _abi.SDB_INVALID_ARGUMENT
    for f in ARRAYS:
        assert call(_without(proj, f)) == _abi.SDB_INVALID_ARGUMENT, f
    assert call(proj, None) == _abi.SDB_INVALID_ARGUMENT  # a NULL out
    assert call(proj, out, wsb - 1) == _abi.SDB_INVALID_ARGUMENT
    if lib.sdb_device_count() == 0:
        assert call(proj) == _abi.SDB_DEVICE_ERROR
        assert call(None) == _abi.SDB_DEVICE_ERROR
