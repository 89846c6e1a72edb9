"""Expected results of sdb_lsm_get_merge and sdb_lsm_scan_merge, computed from the oracle's decoded rows.

get_merge() and scan_merge() restate the rules of include/slatedb_amd.h literally (the reference:
MergeOperatorIterator::merge_with_older_entries, merge_operator.rs:369-448, over GetIterator, db_iter.rs:102-124,
or over the deduplicating MergeIterator, merge_iterator.rs:180-209):
  get   the chain of SSTs, the filters, the block ranges and the block checks of get_cases.Tree.get; every SST
        yields EVERY entry with key == query and seq <= max_seq in physical order; the first entry decides the
        state; while entries are operands the walk goes on; a value ends the chain as its last link, a tombstone
        ends it and is no link (its timestamps are not folded), the end of the SSTs ends it; errors from the SSTs
        up to the one where the chain ended; a link above the newest link's seq fails the query, found per run;
  scan  the candidates of lsm_scan_cases.scan; in the merged order (key ascending, seq descending, earlier SST
        first) the winner of a key is its first visible version; a tombstone winner yields no row; else the links
        are the versions from the winner on up to and including the first value; a tombstone stops the chain, is
        no link, and is folded into the aggregates as the base.
The operator of the tests concatenates, as the reference's StringConcatMergeOperator (reader.rs:489) and
MockMergeOperator (merge_operator.rs:504) do: slatedb_amd.merge.StringConcat.
"""
import collections
import json
import os

import numpy as np

from slatedb_amd import _abi, merge
from slatedb_amd.batch import Batch

from . import get_cases as G
from . import lsm_scan_cases as L
from .scan_cases import EXC, INC, Sst, contains, partitions_covering_range

U64_MAX = G.U64_MAX
OP = merge.StringConcat

# links: (sst, row index into leaves[sst].sst.rows, block), newest first; base: a value (get, scan) or a tombstone
# (scan) ended the chain; sst / block / row: the first entry (get)
MGot = collections.namedtuple("MGot", "state sst block row links base ssts_read ssts_filtered status cts ets")
# rows: (key, links, base, create_ts, expire_ts) in output order
MScan = collections.namedtuple("MScan", "rows status ssts blocks candidates cand_key_bytes")


def _fold_ts(rows, cts, ets):
    """MergeTracker::update over rows' timestamps (merge_operator.rs:289-292)."""
    for r in rows:
        if r[5] is not None:
            cts = r[5] if cts is None else max(cts, r[5])
        if r[6] is not None:
            ets = r[6] if ets is None else min(ets, r[6])
    return cts, ets


def _block_of(s, bs, be, e):
    return max(b for b in range(bs, be) if s.bes[b] <= e)


def get_merge(tree, key, max_seq=None):
    bound = U64_MAX if max_seq is None else int(max_seq)
    read = filt = 0
    first, links, base, ended = None, [], False, False
    fail = lambda st: MGot(_abi.GET_NOT_FOUND, _abi.NO_SST, 0, None, [], False, read, filt, st, None, None)  # noqa: E731
    i0 = 0
    for run in tree.runs:
        err, top = 0, 0  # the run's error; the highest seq of its links
        for i in range(i0, i0 + len(run)):
            l = tree.leaves[i]
            if not l.covers(key):
                continue
            what, (bs, be) = tree.step(i, key)
            if what == "filtered":
                filt += 1
                continue
            if what is not None:
                err = what
                break
            if be <= bs:
                continue
            read += 1
            bad = [l.block_status[b] for b in range(bs, be) if l.block_status.get(b)]
            if bad:
                err = bad[0]
                break
            s = l.sst
            for e in range(s.bes[bs], s.bes[be]):  # physical order
                r = s.rows[e]
                if r[0] != key or r[3] > bound:
                    continue
                blk = _block_of(s, bs, be, e)
                if first is None:
                    first = (i, blk, e)
                if r[4] & _abi.FLAG_TOMBSTONE:
                    ended = True
                    break
                links.append((i, e, blk))
                top = max(top, r[3])
                if not r[4] & _abi.FLAG_MERGE_OPERAND:
                    ended = base = True
                    break
            if ended:
                break
        i0 += len(run)
        if links and top > tree.leaves[links[0][0]].sst.rows[links[0][1]][3]:
            return fail(_abi.SDB_INVALID_SEQUENCE_ORDER)
        if err:
            return fail(err)
        if ended:
            break
    if first is None:
        return MGot(_abi.GET_NOT_FOUND, _abi.NO_SST, 0, None, [], False, read, filt, 0, None, None)
    i, blk, e = first
    flags = tree.leaves[i].sst.rows[e][4]
    if flags & _abi.FLAG_TOMBSTONE:
        return MGot(_abi.GET_DELETED, i, blk, e, [], False, read, filt, 0, None, None)
    cts, ets = _fold_ts([tree.leaves[a].sst.rows[x] for a, x, _ in links], None, None)
    state = _abi.GET_MERGE_OPERAND if flags & _abi.FLAG_MERGE_OPERAND else _abi.GET_FOUND
    return MGot(state, i, blk, e, links, base, read, filt, 0, cts, ets)


def agg_flags(base, cts, ets):
    return ((0 if base else _abi.FLAG_MERGE_OPERAND) | (_abi.FLAG_HAS_CREATE_TS if cts is not None else 0) |
            (_abi.FLAG_HAS_EXPIRE_TS if ets is not None else 0))


def get_columns(tree, g):
    """The sdb_get_out columns of a result (timestamps None when their flag is off)."""
    z = dict(state=g.state, status=g.status, sst=g.sst, block=g.block, val_off=0, val_len=0, seq=0, flags=0,
             create_ts=None, expire_ts=None, ssts_read=g.ssts_read, ssts_filtered=g.ssts_filtered)
    if g.row is None:
        return z
    _, vo, vl, seq, flags, cts, ets = tree.leaves[g.sst].sst.rows[g.row]
    if flags & _abi.FLAG_TOMBSTONE:
        z.update(seq=seq, flags=flags, create_ts=cts, expire_ts=ets)
    else:
        z.update(val_off=vo if vl else 0, val_len=vl, seq=seq, flags=agg_flags(g.base, g.cts, g.ets), create_ts=g.cts,
                 expire_ts=g.ets)
    return z


def link_columns(tree, link):
    i, x, blk = link
    _, vo, vl, seq, flags, cts, ets = tree.leaves[i].sst.rows[x]
    return dict(sst=i, block=blk, val_off=vo if vl else 0, val_len=vl, seq=seq, flags=flags, create_ts=cts, expire_ts=ets)


def folded(tree, key, links, base):
    """merge.fold over a chain's bytes."""
    vals = []
    for i, x, _ in links:
        _, vo, vl = tree.leaves[i].sst.rows[x][:3]
        vals.append(tree.leaves[i].sst.data[vo:vo + vl].tobytes())
    has_value = base and links and not tree.leaves[links[-1][0]].sst.rows[links[-1][1]][4] & _abi.FLAG_MERGE_OPERAND
    return merge.fold(key, vals[:-1] if has_value else vals, vals[-1] if has_value else None, OP)


def scan_merge(tree, rng, max_seq=None, descending=False):
    s, sk, e, ek = L._norm(rng)
    if sk > EXC or ek > EXC:
        return MScan([], _abi.SDB_INVALID_ARGUMENT, [], set(), 0, 0)
    bound = U64_MAX if max_seq is None else int(max_seq)
    ssts = [i for i, l in enumerate(tree.leaves) if L.meets(l, rng)]
    status, blocks, cands = 0, set(), []
    for i in ssts:  # search order
        l, base = tree.leaves[i], int(tree.block_base[i])
        if l.version not in (1, 2):
            status = status or _abi.SDB_INVALID_VERSION
            continue
        bs, be = partitions_covering_range(l.sst.index_keys, s, sk, e, ek)
        be = max(be, bs)
        blocks |= {base + b for b in range(bs, be)}
        for b in range(bs, be):
            if l.block_status.get(b) and not status:
                status = l.block_status[b]
        cands += [(i, x, _block_of(l.sst, bs, be, x)) for x in range(l.sst.bes[bs], l.sst.bes[be])
                  if contains(l.sst.keys[x], s, sk, e, ek)]
    if status:
        return MScan([], status, ssts, blocks, 0, 0)
    ckb = sum(len(tree.leaves[i].sst.keys[x]) for i, x, _ in cands)
    order = sorted((tree.leaves[i].sst.keys[x], -tree.leaves[i].sst.rows[x][3], i, x, b) for i, x, b in cands
                   if tree.leaves[i].sst.rows[x][3] <= bound)
    rows, at = [], 0
    while at < len(order):
        key = order[at][0]
        end = at
        while end < len(order) and order[end][0] == key:
            end += 1
        links, base, cts, ets = [], False, None, None
        for _, _, i, x, b in order[at:end]:
            r = tree.leaves[i].sst.rows[x]
            if r[4] & _abi.FLAG_TOMBSTONE:
                if links:  # the base of a chain: folded (merge_operator.rs:421-425); as a winner it yields nothing
                    base = True
                    cts, ets = _fold_ts([r], cts, ets)
                break
            links.append((i, x, b))
            cts, ets = _fold_ts([r], cts, ets)
            if not r[4] & _abi.FLAG_MERGE_OPERAND:
                base = True
                break
        if links:
            rows.append((key, links, base, cts, ets))
        at = end
    if descending:
        rows.reverse()
    return MScan(rows, 0, ssts, blocks, len(cands), ckb)


def scan_columns(tree, row):
    key, links, base, cts, ets = row
    i, x, _ = links[0]
    _, vo, vl, seq = tree.leaves[i].sst.rows[x][:4]
    return dict(key=key, sst=i, val_off=vo if vl else 0, val_len=vl, seq=seq, flags=agg_flags(base, cts, ets),
                create_ts=cts, expire_ts=ets)


# ------------------------------------------------------------------------------------------------
# The reference's own cases (tests/golden/merge_read_cases.json, written by tests/golden/make_merge_read_cases.py)
# ------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "merge_read_cases.json")
KEPT_GET, KEPT_ITER = 11, 3


def golden():
    return json.load(open(GOLDEN))


def iter_tree(case, version, block_size=4096, split=1):
    """The entries of an iterator case as `split` L0 SSTs (entry j in SST j % split)."""
    runs = []
    for j in range(split):
        es = [(k.encode(), kind, v.encode(), seq, None, ets) for n, (k, kind, v, seq, ets) in enumerate(case["entries"])
              if n % split == j]
        if es:
            runs.append([G.leaf_of(es, version, block_size)])
    return G.Tree(runs)


def iter_expected(case):
    """What a scan yields of the case's expected rows: the first row of every key.  The iterator under test has
    no deduplicating merge below it; a scan's MergeIterator drops what follows a key's first value or tombstone
    (merge_iterator.rs:193-206), and those are the later rows of a key."""
    out, seen = [], set()
    for k, kind, v, seq, ets in case["expected"]:
        if k not in seen:
            seen.add(k)
            out.append((k.encode(), kind, v.encode(), seq, ets))
    return out


# ------------------------------------------------------------------------------------------------
# The tree the device tests read
# ------------------------------------------------------------------------------------------------
def _entries(rng, key_ids, seq, kinds):
    """Sorted entries: 1 to 9 versions per key, mostly operands, short values, some timestamps."""
    es = []
    for k in sorted(key_ids):
        key = b"k%04d" % k
        for _ in range(int(rng.integers(1, 10)) if rng.random() < 0.6 else 1):
            kind = int(rng.choice(kinds))
            es.append((key, kind, bytes(rng.integers(97, 123, int(rng.integers(0, 9)), dtype=np.uint8)), seq,
                       int(rng.integers(0, 2**40)) if rng.random() < 0.3 else None,
                       int(rng.integers(0, 2**40)) if rng.random() < 0.3 else None))
            seq -= 1
    return es, seq


CUT_KEY = b"k0080"


def chain_tree(versions="mixed", seed=5, kinds=(1, 1, 1, 1, 1, 0, 2)):
    """3 L0 SSTs (the middle one and the last with a filter), a sorted run of 3 SSTs cut inside a key's versions,
    an older run of 2 SSTs with values only: blocks of 64 to 128 bytes, so the versions of a key span blocks.
    Even key numbers exist.  versions: 1, 2 or "mixed".  Returns (Tree, the key the cut straddles)."""
    rng = np.random.default_rng(seed)
    ver = (lambda j: versions) if versions != "mixed" else (lambda j: 2 - j % 2)
    seq, runs, j = 10**6, [], 0
    for bs, bloom in ((64, False), (96, True), (128, True)):
        ids = rng.choice(np.setdiff1d(np.arange(0, 160, 2), [80]), 45, replace=False)
        es, seq = _entries(rng, ids, seq, kinds)
        runs.append([G.Leaf(Sst(Batch.from_entries(es), ver(j), bs), bloom)])
        j += 1
    es, seq = _entries(rng, np.arange(0, 160, 2), seq, kinds)
    # the cut: inside the versions of a key that no L0 SST holds, operands on both sides, so its chain crosses the cut
    es = [e for e in es if e[0] != CUT_KEY] + [(CUT_KEY, 1, b"c%d" % x, seq - x, 7 + x if x % 2 else None, None) for x in range(6)]
    seq -= 6
    es.sort(key=lambda e: (e[0], -e[3]))
    c1 = next(i for i, e in enumerate(es) if e[0] == CUT_KEY) + 3
    c2 = G._cut_between_keys(es, 2 * len(es) // 3)
    straddler = es[c1][0]
    run = []
    for (a, b), (bs, bloom) in zip(((0, c1), (c1, c2), (c2, len(es))), ((128, True), (64, False), (96, False))):
        run.append(G.Leaf(Sst(Batch.from_entries(es[a:b]), ver(j), bs), bloom))
        j += 1
    runs.append(run)
    es, seq = _entries(rng, np.arange(0, 200, 2), seq, (0,))
    c1 = G._cut_between_keys(es, len(es) // 2)
    runs.append([G.Leaf(Sst(Batch.from_entries(es[:c1]), ver(j), 64), False),
                 G.Leaf(Sst(Batch.from_entries(es[c1:]), ver(j + 1), 128), True)])
    return G.Tree(runs), straddler


def chain_queries(tree, straddler):
    """About 230 keys: every key number 0..209 (odd: absent; >= 160: only in the oldest run), near misses."""
    return [b"k%04d" % k for k in range(0, 210)] + [b"", b"k", b"zz", straddler + b"\x00", straddler[:-1]] + \
        [straddler] * 3 + [b"k%04d" % k for k in range(0, 24, 2)]


def chain_bounds(tree, keys, seed=3):
    """A max_seq per key: above every version, below every version, or at / just under one of the key's versions."""
    rng = np.random.default_rng(seed)
    out = []
    for q in keys:
        s = G.key_seqs(tree, q)
        c = int(rng.integers(0, 4))
        out.append(U64_MAX if c == 0 or not s else (0 if c == 1 else s[int(rng.integers(0, len(s)))] - (c == 3)))
    return out


def no_operand_tree():
    return L.plain_tree()
