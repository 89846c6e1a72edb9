"""The encoder at its compiled-in limits (tests/encode_cases.py, proven on the CPU by test_encode_cases.py):
every case bit for bit against the oracle through sdb_encode_sst, and the assemblers the device actually
took (sdb_diag_encode_state: the workgroup- and piece-path counters k_blocks leaves in the workspace, the
chain mode and the longest candidate block k_anchor leaves) against the CPU restatement of the routing."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

from . import encode_cases as E
from .test_gpu_parity import assert_same, rt  # noqa: F401

pytestmark = pytest.mark.gpu


class _Got:
    """DeviceSstOutput.to_host() in the shape assert_same reads."""

    def __init__(self, out):
        from slatedb_amd import _abi
        sm = out.summary_host()
        self.status = sm.status
        self.summary = {f: getattr(sm, f) for f, _ in _abi.SstSummary._fields_}
        if sm.status == 0:
            for f, v in out.to_host().items():
                if f != "summary":
                    setattr(self, f, v)


def _state(rt, out, n):  # noqa: F811
    cd = C.CDLL(rt.LIB_PATH)
    cd.sdb_diag_encode_state.restype = None
    cd.sdb_diag_encode_state.argtypes = [C.c_uint64] + [C.c_void_p] * 4
    off = [C.c_uint64() for _ in range(4)]
    cd.sdb_diag_encode_state(n, *[C.byref(o) for o in off])
    word = lambda o: int(out.workspace[o.value:o.value + 4].cpu().numpy().view(np.uint32)[0])
    return dict(zip(("slow_count", "big_count", "wmax", "mode"), map(word, off)))


def device_encode(rt, case):  # noqa: F811
    """The case through sdb_encode_sst on device buffers: (outputs, routing state)."""
    import torch
    b = case.batch
    prm = rt.params(**case.kw)
    out = rt.DeviceSstOutput(b.n, b.logical_bytes(), b.logical_bytes(), prm)
    rt.encode_sst_device(b.to_device("cuda"), out)
    torch.cuda.synchronize()
    return _Got(out), _state(rt, out, b.n)


def check(rt, case):  # noqa: F811
    ref = case.ref()
    got, st = device_encode(rt, case)
    print(case.name, "status", got.status, st)
    assert_same(ref, got, case.name)
    if ref.status == 0:
        _, pieces, workgroup = E.counts(case.routes(ref))
        assert (st["big_count"], st["slow_count"]) == (pieces, workgroup), (case.name, st)
    return ref, got, st


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------
# T first: tombstones whose val_off range is not empty, non-zero first offsets
# ------------------------------------------------------------------------------------------------
def test_t_smallest(rt):  # noqa: F811
    """One ignored byte on one tombstone of a 4 KiB block."""
    check(rt, E.Case("T/smallest", E.t_batch(2, 4096, 1, "middle", 0), **E._fmt_kw(2, 16, 4096, 0)))


@pytest.mark.parametrize("version", [2, 1])
@pytest.mark.parametrize("block_size", [4096, 16384])
def test_t_tombstone_payloads(rt, version, block_size):  # noqa: F811
    routes = set()
    for c in E.t_cases((block_size,), (version,)):
        ref, _, _ = check(rt, c)
        routes |= {r["route"] for r in c.routes(ref)}
    assert routes == {"workgroup", "image" if block_size == 4096 else "pieces"}


@pytest.mark.parametrize("version", [2, 1])
@pytest.mark.parametrize("block_size", [4096, 16384])
def test_t_in_a_set(rt, version, block_size):  # noqa: F811
    """sdb_encode_ssts: one member whose tombstones carry bytes beside one whose do not."""
    import torch
    prm = rt.params(**E._fmt_kw(version, 16, block_size))
    for payload in E.T_PAYLOADS:
        for position in E.T_POSITIONS:
            for off in (0, 15):
                bs = [E.t_batch(version, block_size, payload, position, off), E.t_batch(version, block_size, 0, None, off)]
                dbs = [b.to_device("cuda") for b in bs]
                outs = [rt.DeviceSstOutput(b.n, b.logical_bytes(), b.logical_bytes(), prm, workspace=False) for b in bs]
                ws = rt.ssts_workspace(dbs, prm)
                rt.encode_ssts_device(dbs, outs, prm, ws)
                torch.cuda.synchronize()
                for b, o in zip(bs, outs):
                    assert_same(O.encode_sst(b, O.params(**E._fmt_kw(version, 16, block_size))), _Got(o),
                                "set %d %s off=%d" % (payload, position, off))


@pytest.mark.parametrize("version", [2, 1])
@pytest.mark.parametrize("block_size", [4096, 16384])
def test_t_host_path(rt, version, block_size):  # noqa: F811
    """Encoder.encode_many: the host path copies the batch and rebases both offsets."""
    kw = E._fmt_kw(version, 16, block_size)
    enc = rt.Encoder(rt.params(**kw))
    cases = [c for c in E.t_cases((block_size,), (version,), (10,))]
    for i in range(0, len(cases), 8):
        group = cases[i:i + 8]
        for c, got in zip(group, enc.encode_many([c.batch for c in group])):
            assert_same(c.ref(), got, "host " + c.name)
    enc.close()


# ------------------------------------------------------------------------------------------------
# R: one routing clause at a time
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", E.FORMATS, ids=lambda f: "v%d-ri%d" % f)
def test_r_routing(rt, fmt):  # noqa: F811
    cases = [c for c in E.r_cases() if (c.version, c.kw["restart_interval"]) == fmt]
    assert len(cases) == 25
    seen = set()
    for c in cases:
        ref, _, _ = check(rt, c)
        routes = c.routes(ref)
        seen.add(routes[E.target_block(c, routes)]["route"])
    assert seen == {"image", "pieces", "workgroup"}


# ------------------------------------------------------------------------------------------------
# F: k_facts' lanes, rounds, workgroups and the end of the batch
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.f_lattice_cases(), ids=_ids(E.f_lattice_cases()))
def test_f_lattice(rt, case):  # noqa: F811
    check(rt, case)


def test_f_tails(rt):  # noqa: F811
    for c in E.f_tail_cases():
        check(rt, c)


@pytest.mark.parametrize("case", E.f_geometry_cases(), ids=_ids(E.f_geometry_cases()))
def test_f_geometry(rt, case):  # noqa: F811
    check(rt, case)


def test_f_errors(rt):  # noqa: F811
    for c in E.f_error_cases():
        ref, got, st = check(rt, c)
        assert got.status == c.expect["status"], c.name
        if got.status:
            assert got.summary["first_error_entry"] == c.expect["entry"], c.name
            assert (st["big_count"], st["slow_count"]) == (0, 0), c.name  # k_blocks stops at an error


# ------------------------------------------------------------------------------------------------
# C: chain mode
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("version", [2, 1])
def test_c_chain_mode(rt, version):  # noqa: F811
    cases = [c for c in E.c_cases() if c.version == version]
    assert {c.expect["mode"] for c in cases} == {0, 1}
    for c in cases:
        _, _, st = check(rt, c)
        assert (st["mode"], st["wmax"]) == (c.expect["mode"], c.expect["wmax"]), (c.name, st)
