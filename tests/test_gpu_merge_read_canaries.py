"""Workspace canaries of the merging reads: sdb_lsm_get_merge and sdb_lsm_scan_merge get a workspace of exactly the
size their sdb_*_workspace_bytes function advertises, 257 bytes into a buffer filled with 0xA5.  Every output must
be the model's, and not one byte before or after the workspace may change.  The fill also catches a kernel that
relies on a zeroed workspace."""
import pytest

from . import merge_read_cases as M
from . import test_gpu_merge_reads as T
from .read_harness import canaried_workspace, host, intact, rt  # noqa: F401
from .scan_cases import EXC, INC, U

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("versions", ["mixed", 1])
def test_get_merge_canaries(rt, versions):
    m = T.chain(rt, versions)
    tree, dev, keys = m["tree"], m["dev"], m["queries"]
    big, ws = canaried_workspace(rt, "sdb_lsm_get_merge", dev, len(keys))
    bounds = M.chain_bounds(tree, keys)
    for b in (None, bounds):
        h = host(rt.lsm_get_merge_device(dev, None, keys, max_seq=b, workspace=ws, cap_links=2048, fill=T.SENTINEL))
        T.check_get(tree, keys, b, h)
        intact(big, ws.numel())


@pytest.mark.parametrize("desc", [False, True])
def test_scan_merge_canaries(rt, desc):
    m = T.chain(rt, "mixed")
    tree, dev = m["tree"], m["dev"]
    rngs = [(None, U, None, U), (b"k0010", INC, b"k0050", EXC), (M.CUT_KEY, INC, M.CUT_KEY, INC), (b"k0100", EXC, None, U)]
    exp = [M.scan_merge(tree, r) for r in rngs]
    cand = (sum(e.candidates for e in exp), sum(e.cand_key_bytes for e in exp))  # exact: the arrays end where the workspace ends
    rows = [r for e in exp for r in e.rows]
    cap = (len(rows), sum(len(r[0]) for r in rows))
    big, ws = canaried_workspace(rt, "sdb_lsm_scan_merge", dev, len(rngs), cand)
    h = host(rt.lsm_scan_merge_device(dev, rngs, descending=desc, workspace=ws, cand=cand, cap=cap,
                                      cap_links=sum(len(r[1]) for r in rows), fill=T.SENTINEL))
    T.check_scan(tree, rngs, None, desc, h)
    intact(big, ws.numel())
