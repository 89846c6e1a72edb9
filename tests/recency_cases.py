"""Expected results of sdb_lsm_scan_recency: Db::scan_prefix_by_recency over the MemTree of tests/mem_scan_cases.py.

scan_recency() restates rules R1-R6 of include/slatedb_amd.h literally (the reference:
Reader::scan_prefix_by_recency_with_options, reader.rs:322-428; DbRecencyIterator, db_iter.rs:376-442):
  R1  the sources are the tables with a row of the range, then the runs with a participating SST, newest first; a
      sorted run is one source, an L0 SST a run of one; descending a run's SSTs are walked last to first;
  R2  a pair's rows are its candidates as sdb_lsm_scan_mem stages them (participation, filter, view range, block
      clip, a table's stretch) at or below max_seq; tombstones and operands are rows;
  R3  ascending the physical order; descending the key groups reversed, a group's versions newest first, per SST;
  R4  the range's rows are the concatenation over the walk order;
  R5  with a limit L the first L rows; a source is opened iff the sources before it gave fewer than L rows; only an
      opened source fails the range, the first failing SST in walk order with its lowest block; a failing range has no
      rows; a filtered-out SST is never opened;
  R6  every pair without an error stages its candidates, reached or not; when they do not fit (fits=False) the
      status is that of limit 0 and nothing counts as read.
brute() is independent of it: per source every row of the range, sorted by R3, concatenated, truncated.
"""
import collections
import json
import os

from oracle import oracle as O
from slatedb_amd import _abi

from . import filtered_read_cases as F
from . import get_cases as G
from . import lsm_scan_cases as L
from . import mem_scan_cases as S
from . import projected_read_cases as P
from .scan_cases import EXC, INC, U, contains, partitions_covering_range

U64_MAX = G.U64_MAX

# rows: (key, source), source ("t", table, row) or ("s", sst, row, 0); ssts / tables / filtered / blocks / candidates /
# cand_key_bytes as mem_scan_cases.MemScan; sources_read, visible: R5
RecScan = collections.namedtuple("RecScan", "rows status ssts tables blocks candidates cand_key_bytes filtered sources_read visible")


def prefix_range(p):
    """BytesRange::from_prefix."""
    if not p:
        return (None, U, None, U)
    end = p.rstrip(b"\xff")
    return (p, INC, end[:-1] + bytes([end[-1] + 1]), EXC) if end else (p, INC, None, U)


def _ruled_out(leaf, rng, V, prefix, probe_len):
    """F1-F3 / P4: a leaf of filtered_read_cases under its policy, a plain leaf under the whole-key policy."""
    if hasattr(leaf, "policy"):
        q, pl = P.pair_query(rng, V, prefix, probe_len)
        return F.ruled_out(leaf, q, pl)
    if leaf.bloom is None:
        return False
    q = P.pair_query(rng, V, prefix, probe_len)[0]
    return q is not None and not q[1] and not O.might_contain(leaf.bloom, G.NUM_PROBES, q[0])


def ordered(rows_of, idx, descending):
    """R3: the rows idx (physical order) of one table or SST; descending the key groups reversed."""
    if not descending:
        return list(idx)
    groups = []
    for i in idx:
        if groups and rows_of[groups[-1][0]][0] == rows_of[i][0]:
            groups[-1].append(i)
        else:
            groups.append([i])
    return [i for g in reversed(groups) for i in g]


def scan_recency(mt, rng, prefix=None, max_seq=None, limit=0, descending=False, visible=None, probe_len=None, fits=True):
    s, sk, e, ek = L._norm(rng)
    if sk > EXC or ek > EXC:
        return RecScan([], _abi.SDB_INVALID_ARGUMENT, [], [], set(), 0, 0, [], 0, 0)
    bound = U64_MAX if max_seq is None else int(max_seq)
    tree = mt.tree
    # the pairs: per source unit its status and its candidates in physical order
    sources, tabs, ssts, filtered, blocks = [], [], [], [], set()
    ncand = ckb = 0
    for t, table in enumerate(mt.tables):
        g0, g1 = S.stretch(table, rng)
        if g1 > g0:
            tabs.append(t)
            sources.append([(0, table.rows, [("t", t, i) for i in range(g0, g1)])])
    i0 = 0
    for run in tree.runs:
        units = []
        for i in range(i0, i0 + len(run)):
            l = tree.leaves[i]
            V = P.view_range(rng, None if visible is None else visible[i])
            if V is None or not L.meets(l, V):
                continue
            if _ruled_out(l, rng, V, prefix, probe_len):
                filtered.append(i)
                continue
            ssts.append(i)
            if l.version not in (1, 2):
                units.append((_abi.SDB_INVALID_VERSION, l.sst.rows, []))
                continue
            bs, be = partitions_covering_range(l.sst.index_keys, *V)
            be = max(be, bs)
            blocks |= {int(tree.block_base[i]) + b for b in range(bs, be)}
            st = next((l.block_status[b] for b in range(bs, be) if l.block_status.get(b)), 0)
            cands = [] if st else [("s", i, x, 0) for x in range(l.sst.bes[bs], l.sst.bes[be]) if contains(l.sst.keys[x], *V)]
            units.append((st, l.sst.rows, cands))
        i0 += len(run)
        if units:
            sources.append(units[::-1] if descending else units)
    for units in sources:  # R6: reached or not
        for st, _, cands in units:
            ncand += len(cands)
            ckb += sum(len(mt.row_of(c)[0]) for c in cands)
    if not fits:
        status = next((st for units in sources for st, _, _ in units if st), 0)
        return RecScan([], status, ssts, tabs, blocks, ncand, ckb, filtered, 0, 0)
    rows, status, nread, seen = [], 0, 0, 0
    for units in sources:  # R5: the walk
        if limit and len(rows) >= limit:
            break
        nread += 1
        status = next((st for st, _, _ in units if st), 0)
        for _, rows_of, cands in units:
            vis = [c for c in cands if rows_of[c[2]][3] <= bound]
            seen += len(vis)
            by_row = {c[2]: c for c in vis}
            rows += [(rows_of[i][0], by_row[i]) for i in ordered(rows_of, [c[2] for c in vis], descending)]
        if status:
            return RecScan([], status, ssts, tabs, blocks, ncand, ckb, filtered, nread, 0)
    return RecScan(rows[:limit] if limit else rows, 0, ssts, tabs, blocks, ncand, ckb, filtered, nread, seen)


def brute(mt, rng, max_seq=None, limit=0, descending=False):
    """Independent of scan_recency(): per source ALL its rows whose key the range contains, at or below the bound,
    sorted by key (descending: reversed) and then seq descending, concatenated, truncated -> [(key, source)]."""
    s, sk, e, ek = L._norm(rng)
    bound = U64_MAX if max_seq is None else int(max_seq)
    units = [[("t", t, i) for i in range(len(tb.rows))] for t, tb in enumerate(mt.tables)]
    i0 = 0
    for run in mt.tree.runs:
        ssts = [[("s", i, x, 0) for x in range(len(mt.tree.leaves[i].sst.rows))] for i in range(i0, i0 + len(run))]
        units += ssts[::-1] if descending else ssts
        i0 += len(run)
    out = []
    for unit in units:
        keep = [c for c in unit if contains(mt.row_of(c)[0], s, sk, e, ek) and mt.row_of(c)[3] <= bound]
        keep.sort(key=lambda c: (-mt.row_of(c)[3], c[2]))  # newest first, then the physical order (stable below)
        keep.sort(key=lambda c: mt.row_of(c)[0], reverse=descending)
        out += [(mt.row_of(c)[0], c) for c in keep]
    return out[:limit] if limit else out


def first_per_key(rows, mt):
    """The relation with Db::scan on a well-formed tree: the first occurrence per key in walk order, tombstones
    dropped, in key order."""
    first = {}
    for key, src in rows:
        first.setdefault(key, src)
    return [(k, first[k]) for k in sorted(first) if not mt.row_of(first[k])[4] & _abi.FLAG_TOMBSTONE]


def columns(mt, row):
    """The row's columns as S.columns, with the stored flags: a tombstone has no value."""
    z = S.columns(mt, row)
    if z["flags"] & _abi.FLAG_TOMBSTONE:
        z["val_off"] = z["val_len"] = 0
    return z


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "recency_cases.json")
KEPT_CASES = 7


def golden_cases():
    return json.load(open(GOLDEN))["cases"]


def kind_of(flags):
    return 2 if flags & _abi.FLAG_TOMBSTONE else (1 if flags & _abi.FLAG_MERGE_OPERAND else 0)


def layered_tree(seed, version=2, block_size=64, ntab=2, nl0=2, run_ssts=(2, 3), nkeys=24, kinds=(0, 0, 1, 2), tiny=False):
    """A small well-formed tree: every newer source holds higher seqs.  ntab tables, nl0 L0 SSTs and sorted runs of
    run_ssts SSTs (cut between keys or inside a key's versions), 1 to 3 versions per key, keys with a proper-prefix
    neighbour.  tiny: at most 8 rows per table and SST, values of at most 3 bytes (the device tests' shapes)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    pool = [b"px:%02d" % i for i in range(nkeys)] + [b"px:03\x00", b"px:", b"py:0", b"pw:9"]
    nsrc = ntab + nl0 + len(run_ssts)
    seq = 1000 * (nsrc + 1)

    def entries():
        nonlocal seq
        es = []
        for k in sorted(set(pool[int(j)] for j in rng.integers(0, len(pool), int(rng.integers(3, 5 if tiny else 14))))):
            for _ in range(int(rng.integers(1, 3 if tiny else 4))):
                seq -= 1
                kind = int(rng.choice(kinds))
                es.append((k, kind, b"" if kind == 2 else bytes(rng.integers(97, 123, int(rng.integers(0, 4 if tiny else 9)), dtype=np.uint8)),
                           seq, None, int(rng.integers(1, 2**40)) if rng.random() < 0.2 else None))
        return es

    tables = [S.Table(entries()) for _ in range(ntab)]
    runs = [[G.leaf_of(entries(), version, block_size)] for _ in range(nl0)]
    for n in run_ssts:
        es = sorted(entries() + entries(), key=lambda x: (x[0], -x[3]))
        cuts = sorted(set(int(c) for c in rng.integers(1, max(2, len(es) - 1), n - 1)))
        parts = [es[a:b] for a, b in zip([0] + cuts, cuts + [len(es)]) if b > a]
        runs.append([G.leaf_of(p, version, block_size) for p in parts])
    return S.MemTree(tables, G.Tree(runs))
