"""The C ABI of the ranged compaction (sdb_compactor_run_ssts_ranged, sdb_compactor_range_stats): the symbols, the
struct layouts against the header, the host checks of rule R7 and the no-device path; and the host side of a ranged
job: the expected-value model of tests/ranged_compaction_cases.py over the planner's ranges, and the planner's
effective_range.  No device is needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import pytest

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd import subcompaction as S

from . import ranged_compaction_cases as R
from .test_subcompaction import k, merged_entries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "slatedb_amd.h")
NEW = ("sdb_compactor_run_ssts_ranged", "sdb_compactor_range_stats")


@pytest.fixture(scope="module")
def lib():
    from slatedb_amd import runtime
    return runtime.lib()


def test_symbols(lib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "slatedb_amd", "libslatedb_amd.so")]).decode()
    exported = set(re.findall(r" T (sdb_\w+)", out))
    assert set(NEW) <= exported and set(NEW) <= set(_abi.SIGNATURES)
    hdr = open(HDR).read()
    for name in NEW:
        assert re.search(r"\b%s\(" % name, hdr), name
    for rule in range(1, 9):
        assert re.search(r"\bR%d\. " % rule, hdr), rule
    assert lib.sdb_abi_version() == 2  # no existing struct changed


def test_struct_layouts_match_header():
    structs = {"sdb_compaction_view": _abi.CompactionView, "sdb_range_job_stats": _abi.RangeJobStats,
               "sdb_compaction_input": _abi.CompactionInput}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "%s"' % HDR, "int main(void){"]
    for cname, py in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in py._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append("return 0;}")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.c"), os.path.join(d, "l")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c11", "-o", exe, src])
        out = dict(l.split() for l in subprocess.check_output([exe]).decode().splitlines())
    for cname, py in structs.items():
        assert int(out[cname]) == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert int(out["%s.%s" % (cname, f)]) == getattr(py, f).offset, (cname, f)


def _ranges(n, p):
    return _abi.ScanRanges(n, p, p, p, p, p, p)


def _without(rg, field):
    vals = {f: getattr(rg, f) for f, _ in _abi.ScanRanges._fields_}
    vals[field] = None
    return _abi.ScanRanges(*[vals[f] for f, _ in _abi.ScanRanges._fields_])


ARRAYS = [f for f, _ in _abi.ScanRanges._fields_ if f != "n"]


def test_host_checks(lib):
    """R7 on the host: each is SDB_INVALID_ARGUMENT from the call, with no handle and no device; a well-formed call
    then reports the missing device."""
    keep = [(C.c_uint64 * 64)() for _ in range(4)]
    p = [C.addressof(x) for x in keep]
    ret, prm, ns = O.retention(), O.params(sst_type=_abi.SST_COMPACTED), C.c_uint32(7)

    def view(data=p[0], boff=p[0], ik=p[1], iko=p[1], nb=4):
        return _abi.CompactionView(_abi.CompactionInput(data, boff, nb, 1, 1, 1), ik, iko)

    def call(job, proj, views=None, n=2):
        cv = (_abi.CompactionView * 2)(*(views or [view(), view()]))
        return lib.sdb_compactor_run_ssts_ranged(None, cv, n, None, n, 2, None if job is None else C.byref(job),
                                                 None if proj is None else C.byref(proj), C.byref(ret),
                                                 _abi.MERGE_BATCH_FN(), None, C.byref(prm), 1 << 20, None, C.byref(ns))

    job, proj = _ranges(1, p[2]), _ranges(2, p[3])
    bad = _abi.SDB_INVALID_ARGUMENT
    assert call(_ranges(0, p[2]), proj) == bad and call(_ranges(2, p[2]), proj) == bad  # job_range->n != 1
    assert call(job, _ranges(1, p[3])) == bad and call(job, _ranges(3, p[3])) == bad    # proj->n != ninputs
    for f in ARRAYS:  # a NULL array inside a non-NULL struct
        assert call(_without(job, f), proj) == bad, f
        assert call(job, _without(proj, f)) == bad, f
        assert call(_without(job, f), None) == bad and call(None, _without(proj, f)) == bad, f
    for kw in (dict(ik=None), dict(iko=None), dict(data=None), dict(boff=None)):  # num_blocks > 0 without its arrays
        assert call(job, proj, [view(), view(**kw)]) == bad, kw
    if lib.sdb_device_count() == 0:  # after the host checks, without a device
        for j, q in ((job, proj), (None, proj), (job, None), (None, None)):
            assert call(j, q) == _abi.SDB_DEVICE_ERROR
        assert call(job, proj, [view(), view(ik=None, iko=None, data=None, boff=None, nb=0)]) == _abi.SDB_DEVICE_ERROR
    st = _abi.RangeJobStats()
    assert lib.sdb_compactor_range_stats(None, C.byref(st)) == bad


def test_range_bounds():
    U, INC, EXC = _abi.BOUND_UNBOUNDED, _abi.BOUND_INCLUDED, _abi.BOUND_EXCLUDED
    assert S.range_bounds(S.UNBOUNDED) == (None, U, None, U)
    assert S.range_bounds(S.KeyRange(b"a", b"c")) == (b"a", INC, b"c", EXC)
    assert S.range_bounds(S.KeyRange(None, b"c")) == (None, U, b"c", EXC)
    assert S.range_bounds(S.KeyRange(b"a", None)) == (b"a", INC, None, U)
    for key in (b"", b"a", b"b", b"c", b"d"):
        for rng in (S.KeyRange(b"a", b"c"), S.KeyRange(None, b"c"), S.KeyRange(b"a", None), S.UNBOUNDED):
            s, sk, e, ek = S.range_bounds(rng)
            assert R.contains(key, s or b"", sk, e or b"", ek) == rng.contains(key)


def test_clipped_ranges_concatenate_to_the_unsplit_job():
    """Planner ranges -> R1-R3 on the host -> the oracle's compaction: the ranges' merged streams concatenate to the
    unsplit job's, every input row lands in exactly one range, and only boundary blocks are read twice."""
    job = R.small_job()
    ret, prm = O.retention(min_seq=3000, compaction_start_ts=1000, filter_tombstone=True), O.params(block_size=512)
    ranges = S.plan_subcompaction_ranges(R.metas(job), 4)
    assert len(ranges) >= 2
    (whole, wsm, _, _), wst = R.expected(job, ret, prm, R.MAX_SST)
    assert wsm.status == 0 and wst["blocks_checked"] == wst["blocks_total"] and wst["entries_in"] == wst["entries_decoded"]
    got, rows, blocks = [], 0, 0
    for x in ranges:
        (part, sm, _, _), st = R.expected(job, ret, prm, R.MAX_SST, job_range=S.range_bounds(x))
        assert sm.status == 0 and sm.num_in == st["entries_in"]
        got += merged_entries(part)
        rows += st["entries_in"]
        blocks += st["blocks_checked"]
    assert got == merged_entries(whole) and rows == wst["entries_in"]
    # a block at a boundary may be read by both neighbours: at most one per input and boundary
    assert wst["blocks_total"] <= blocks <= wst["blocks_total"] + len(job.inputs) * (len(ranges) - 1)


def test_planner_clips_anchors_to_the_effective_range():
    """subcompaction.rs:155-160 (test_sample_anchors_clips_to_projected_effective_range at the planner's level): the
    anchors of a projected input outside its effective range do not weigh in."""
    keys, offs = [k(10 * i) for i in range(8)], [100 * i for i in range(8)]
    other = [k(10 * i + 5) for i in range(8)]
    eff = S.KeyRange(k(20), k(50))
    plain = [S.SstMeta(keys, offs, 800), S.SstMeta(other, offs, 800)]
    proj = [S.SstMeta(keys, offs, 800, effective_range=eff), S.SstMeta(other, offs, 800)]
    assert plain[0].effective_range is None
    anchors = [a for a in S.sample_anchors(keys, offs, 800) if eff.contains(a[0])] + S.sample_anchors(other, offs, 800)
    assert [a[0] for a in anchors[:3]] == [k(20), k(30), k(40)] and len(anchors) == 11
    want = S.select_boundaries(anchors, 4, 800)
    assert S.plan_subcompaction_ranges(proj, 4) == want
    assert S.plan_subcompaction_ranges(plain, 4) == S.select_boundaries(
        S.sample_anchors(keys, offs, 800) + S.sample_anchors(other, offs, 800), 4, 800)
    assert S.plan_subcompaction_ranges(proj, 4) != S.plan_subcompaction_ranges(plain, 4)
