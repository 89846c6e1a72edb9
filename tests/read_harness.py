"""What the GPU tests of the tree reads (sdb_lsm_get*, sdb_lsm_scan*, sdb_lsm_scan_recency) share: the runtime fixture,
device trees and tables, one host() for every family's result dict, the column comparison, the scan checks' common
core, and what a test hands the wrappers to control their outputs and workspace: allocators for alloc= (see
slatedb_amd.runtime._read_output) and a canaried workspace.  The calls themselves are always the runtime's: a test
marshals nothing.  What is tied to one *_cases model (check, check_get, check_scan, ...) stays in the test module
that owns it."""
import numpy as np
import pytest

from . import get_cases as G

U64_MAX = G.U64_MAX
U32_COLS = ("sst", "block", "table", "val_len", "ssts_read", "ssts_filtered", "status")
LEAD, TAIL = 257, 512  # the bytes around a canaried workspace


@pytest.fixture(scope="module")
def rt():
    from slatedb_amd import runtime
    runtime.require_device()
    return runtime


# ------------------------------------------------------------------------------------------------
# Trees and tables on the device
# ------------------------------------------------------------------------------------------------
def to_dev(a, device="cuda"):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    if not a.size:
        a = np.zeros(16, a.dtype)
    return torch.from_numpy(a).to(device)


def view_of(leaf, data=None, block_off=None, plain=False, device="cuda"):
    """The view of a leaf, as lsm_tree_device takes it; a leaf of filtered_read_cases brings its policy and its
    filter's probes.  plain: no filter and no policy (what the unfiltered calls' tests of a filtered tree read)."""
    s = leaf.sst
    dv = lambda a: to_dev(a, device)  # noqa: E731
    v = {"data": dv(np.concatenate([s.data if data is None else data, np.zeros(64, np.uint8)])),
         "block_off": dv(s.block_off if block_off is None else block_off), "num_blocks": s.nb,
         "index_keys": dv(s.ik_bytes), "index_key_off": dv(s.ik_off), "sst_version": leaf.version,
         "first_key": leaf.first_key, "last_key": leaf.last_key}
    if plain:
        return v
    if hasattr(leaf, "policy"):
        v["policy"] = tuple(leaf.policy)
    if leaf.bloom is not None:
        v.update(bloom=dv(leaf.bloom), bloom_len=len(leaf.bloom), num_probes=getattr(leaf, "num_probes", G.NUM_PROBES))
    return v


def device_tree(rt, tree, views=None, plain=False):
    return rt.lsm_tree_device(views or [view_of(l, plain=plain) for l in tree.leaves], [len(r) for r in tree.runs])


def dev_tree(rt, tree, views=None):
    """device_tree, and the tree without SSTs."""
    return device_tree(rt, tree, views) if tree.leaves else rt.lsm_tree_device([], [])


def dev_tables(rt, tables):
    return rt.mem_tables_device([rt.DeviceRun.from_host(t.run) for t in tables])


# ------------------------------------------------------------------------------------------------
# Results on the host
# ------------------------------------------------------------------------------------------------
def host(res):
    """Every tensor of a result dict as a numpy array, and the summaries it holds word by word: summary under sum_*
    (LSM_SCAN_SUMMARY for a scan, GET_SUMMARY for a get), chain_summary under csum_*, num_filtered as
    sum_num_filtered."""
    import torch
    from slatedb_amd import runtime
    if any(v.is_cuda for k, v in res.items() if not k.startswith("_")):
        torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in res.items() if not k.startswith("_")}
    words = [("sum_", "summary", runtime.LSM_SCAN_SUMMARY if "range_entry_start" in h else runtime.GET_SUMMARY)]
    if "chain_summary" in h:
        words.append(("csum_", "chain_summary", runtime.CHAIN_SUMMARY))
    for prefix, key, names in words:
        for i, f in enumerate(names):
            h[prefix + f] = int(h[key][i]) & (0xFFFFFFFF if f == "status" else U64_MAX)
    if "num_filtered" in h:
        h["sum_num_filtered"] = int(h["num_filtered"][0])
    return h


def u64(a, f):
    a = a.astype(np.int64).astype(np.uint64)
    return a & np.uint64(0xFFFFFFFF) if f in U32_COLS else a


def compare(names, cols, have, what):
    """The columns `names` and the timestamps of the model's cols against have(field)[:len(cols)]."""
    n = len(cols)
    for f in names:
        want = np.array([c[f] for c in cols], np.uint64)
        got = u64(have(f)[:n], f)
        bad = np.nonzero(want != got)[0]
        assert not bad.size, (what, f, int(bad[0]), cols[int(bad[0])], int(want[bad[0]]), int(got[bad[0]]))
    for f in ("create_ts", "expire_ts"):
        want = np.array([c[f] if c[f] is not None else 0 for c in cols], np.int64)
        assert (have(f)[:n] == want).all(), (what, f)


def check_get_summary(got, failed, h):
    """The get summary against the model's results; failed: the queries that count as failed."""
    from slatedb_amd import _abi
    count = lambda st: sum(1 for g in got if g.state == st)  # noqa: E731
    assert h["sum_num_found"] == count(_abi.GET_FOUND) and h["sum_num_deleted"] == count(_abi.GET_DELETED)
    assert h["sum_num_merge"] == count(_abi.GET_MERGE_OPERAND) and h["sum_num_failed"] == len(failed)
    assert h["sum_num_not_found"] == count(_abi.GET_NOT_FOUND) - len(failed)
    assert h["sum_status"] == (got[failed[0]].status if failed else 0)


def totals(exp):
    """((candidates, candidate key bytes), (rows, key bytes)) of a call's model results: its exact capacities."""
    return ((sum(e.candidates for e in exp), sum(e.cand_key_bytes for e in exp)),
            (sum(len(e.rows) for e in exp), sum(len(r[0]) for e in exp for r in e.rows)))


def check_scan_core(exp, h):
    """What every scan family checks alike against its model's results (rows that start with their key):
    range_entry_start, the summary's counts and status, key_off and key_arena.  Returns the rows."""
    rows = [r for e in exp for r in e.rows]
    starts = np.concatenate([[0], np.cumsum([len(e.rows) for e in exp])]).astype(np.int64)
    assert (h["range_entry_start"][:len(exp) + 1].astype(np.int64) == starts).all()
    failed = [q for q, e in enumerate(exp) if e.status]
    (nc, ckb), (ne, kb) = totals(exp)
    assert h["sum_num_entries"] == ne and h["sum_key_bytes"] == kb
    assert h["sum_num_candidates"] == nc
    assert h["sum_candidate_key_bytes"] == ckb
    assert h["sum_num_failed_ranges"] == len(failed)
    assert h["sum_status"] == (exp[failed[0]].status if failed else 0)
    ko = h["key_off"][:ne + 1].astype(np.int64)
    assert (ko == np.concatenate([[0], np.cumsum([len(r[0]) for r in rows])])).all()
    assert h["key_arena"][:kb].tobytes() == b"".join(r[0] for r in rows)
    return rows


# ------------------------------------------------------------------------------------------------
# Allocators for the wrappers' alloc=
# ------------------------------------------------------------------------------------------------
class Filled:
    """Every output starts as `byte`, whatever fill the call asks for, with room behind the capacity the call is
    given (8 rows or links, 64 key bytes), so that "nothing past the capacity" can be checked."""

    def __init__(self, byte, device="cuda"):
        self.byte, self.device = byte, device

    def __call__(self, name, count, dtype, fill):
        import torch
        exact = name.startswith(("range_", "_")) or name.endswith(("_start", "summary")) or name in ("key_off", "num_filtered")
        pad = 0 if exact else 64 if name == "key_arena" else 8
        return torch.full((max(count + pad, 1) * dtype.itemsize,), self.byte, dtype=torch.uint8, device=self.device).view(dtype)


def untouched(h, fields, byte):
    return all((h[f].view(np.uint8) == byte).all() for f in fields)


class Guard:
    """Every output of exactly its size, 0xA5 in it and in the guard bytes before and after it; a workspace the call
    asks for starts at an odd address."""
    TAIL = 256

    def __init__(self, device="cuda"):
        self.device, self.bufs = device, []

    def alloc(self, n, dtype, lead=256):
        import torch
        nb = n * dtype.itemsize
        big = torch.full((lead + nb + self.TAIL,), 0xA5, dtype=torch.uint8, device=self.device)
        self.bufs.append((big, lead, nb))
        return big[lead:lead + nb].view(dtype) if lead % 8 == 0 else big[lead:lead + nb]

    def __call__(self, name, count, dtype, fill):
        return self.alloc(count, dtype, LEAD if name == "_ws" else 256)

    def check(self):
        import torch
        if self.device != "cpu":
            torch.cuda.synchronize()
        for big, lead, nb in self.bufs:
            assert bool((big[:lead] == 0xA5).all()) and bool((big[lead + nb:] == 0xA5).all()), (lead, nb)


def canaried_workspace(rt, entry, tree, n, cand=(0, 0), merge=False, tables=None, byte=0xA5):
    """(big, ws): a workspace of exactly the size entry's sizer advertises for the shape, LEAD bytes into a buffer
    filled with `byte` (which also catches a kernel that relies on a zeroed workspace) and TAIL bytes before its end."""
    import torch
    wsb = rt.read_workspace_bytes(entry, tree, n, cand, merge, tables)
    big = torch.full((LEAD + wsb + TAIL,), byte, dtype=torch.uint8, device=tree["device"])
    return big, big[LEAD:LEAD + wsb]


def intact(big, wsb, byte=0xA5):
    import torch
    if big.is_cuda:
        torch.cuda.synchronize()
    assert bool((big[:LEAD] == byte).all()), "bytes before the workspace changed"
    assert bool((big[LEAD + wsb:] == byte).all()), "bytes after the workspace changed"
