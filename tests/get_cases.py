"""Expected results of sdb_lsm_get, computed from the oracle's ascending block decode.

Tree.get restates the rules of include/slatedb_amd.h literally (the reference: GetIterator::from_lsm_tree,
db_iter.rs:79-124, over build_l0_point_iters / build_sr_point_iters, segment_iterator.rs:312-353):
  1. the chain of a key: over the runs in order, the SSTs i of the run with first_key[i] <= key <= last_key[i]
     (contiguous in a well-formed sorted run: tables_covering_point_key, db_state.rs:540-596);
  2. per SST: the bloom filter may rule it out; else the blocks partitions_covering_range([key, key]); every
     block of them is checked, the lowest failing one fails the query; then the first entry in physical order
     with key == query and seq <= max_seq (FilterIterator::new_with_max_seq, filter_iterator.rs:22-48);
  3. value -> FOUND, tombstone -> DELETED, merge operand -> MERGE_OPERAND (MERGE_OPERATOR_MISSING), an
     exhausted chain -> NOT_FOUND;
  4. errors only from SSTs at or before the deciding one, never from a filtered one.
"""
import collections
import json
import os

import numpy as np

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd.batch import Batch

from .scan_cases import INC, Sst, partitions_covering_range

NUM_PROBES = O.optimal_num_probes(10)  # O.params' default bits per key
U64_MAX = (1 << 64) - 1

Got = collections.namedtuple("Got", "state sst block row ssts_read ssts_filtered status need")


class EmptySst:
    """An SST without blocks (num_blocks == 0): no entries, no first / last key."""
    version, nb, rows, keys, bes, index_keys = 2, 0, [], [], [0], []
    data = np.zeros(0, np.uint8)
    block_off = np.zeros(1, np.uint64)
    ik_bytes = np.zeros(0, np.uint8)
    ik_off = np.zeros(1, np.uint64)


class Leaf:
    """One SST of a tree: the oracle-encoded Sst, whether its filter is used, and the blocks a test broke
    ({block: status})."""

    def __init__(self, sst, bloom=False, block_status=None, version=None):
        self.sst = sst
        self.bloom = sst.enc.bloom if bloom else None
        self.block_status = block_status or {}
        self.version = sst.version if version is None else version  # what the view claims
        self.first_key = sst.keys[0] if sst.keys else b""
        self.last_key = sst.keys[-1] if sst.keys else b""

    def covers(self, key):
        return bool(self.sst.keys) and self.first_key <= key <= self.last_key


def leaf_of(entries, version, block_size, bloom=False):
    """entries: (key, kind, value, seq, create_ts, expire_ts); sorted here as an SST holds them."""
    es = sorted(entries, key=lambda e: (e[0], -e[3]))
    return Leaf(Sst(Batch.from_entries(es), version, block_size), bloom)


class Tree:
    """runs: lists of Leaf, newest run first; an L0 SST is a run of one."""

    def __init__(self, runs):
        self.runs = [list(r) for r in runs]
        self.leaves = [l for r in self.runs for l in r]
        self.block_base = np.concatenate([[0], np.cumsum([l.sst.nb for l in self.leaves])]).astype(np.int64)

    def chain(self, key):
        """Indices into self.leaves, rule 1."""
        out, i0 = [], 0
        for run in self.runs:
            cov = [j for j, l in enumerate(run) if l.covers(key)]
            assert cov == list(range(cov[0], cov[0] + len(cov))) if cov else True, "covering SSTs are contiguous"
            out += [i0 + j for j in cov]
            i0 += len(run)
        return out

    def step(self, i, key):
        """("filtered" | status | None, (start block, end block)) of leaf i for a key, rule 2."""
        l = self.leaves[i]
        if l.bloom is not None and not O.might_contain(l.bloom, NUM_PROBES, key):
            return "filtered", (0, 0)
        if l.version not in (1, 2):
            return _abi.SDB_INVALID_VERSION, (0, 0)
        return None, partitions_covering_range(l.sst.index_keys, key, INC, key, INC)

    def get(self, key, max_seq=None):
        bound = U64_MAX if max_seq is None else int(max_seq)
        read = filt = 0
        need = set()  # tree blocks the chain needs up to the decision
        fail = lambda st: Got(_abi.GET_NOT_FOUND, _abi.NO_SST, 0, None, read, filt, st, need)  # noqa: E731
        for i in self.chain(key):
            what, (bs, be) = self.step(i, key)
            if what == "filtered":
                filt += 1
                continue
            if what is not None:
                return fail(what)
            if be <= bs:
                continue
            read += 1
            l, base = self.leaves[i], int(self.block_base[i])
            need |= {base + b for b in range(bs, be)}
            for b in range(bs, be):
                if l.block_status.get(b):
                    return fail(l.block_status[b])
            s = l.sst
            for e in range(s.bes[bs], s.bes[be]):  # physical order
                k, _, _, seq, flags = s.rows[e][:5]
                if k == key and seq <= bound:
                    block = max(b for b in range(bs, be) if s.bes[b] <= e)
                    if flags & _abi.FLAG_TOMBSTONE:
                        state, st = _abi.GET_DELETED, 0
                    elif flags & _abi.FLAG_MERGE_OPERAND:
                        state, st = _abi.GET_MERGE_OPERAND, _abi.SDB_MERGE_OPERATOR_MISSING
                    else:
                        state, st = _abi.GET_FOUND, 0
                    return Got(state, i, block, e, read, filt, st, need)
        return Got(_abi.GET_NOT_FOUND, _abi.NO_SST, 0, None, read, filt, 0, need)

    def covering_blocks(self, key):
        """Tree blocks of every unfiltered, usable SST of the whole chain: what an eager call may check."""
        out = set()
        for i in self.chain(key):
            what, (bs, be) = self.step(i, key)
            if what is None:
                out |= {int(self.block_base[i]) + b for b in range(bs, be)}
        return out

    def columns(self, g):
        """The sdb_get_out columns of a result: dict field -> value (timestamps None when their flag is off)."""
        z = dict(state=g.state, status=g.status, sst=g.sst, block=g.block, val_off=0, val_len=0, seq=0, flags=0,
                 create_ts=None, expire_ts=None, ssts_read=g.ssts_read, ssts_filtered=g.ssts_filtered)
        if g.row is not None:
            _, vo, vl, seq, flags, cts, ets = self.leaves[g.sst].sst.rows[g.row]
            if flags & _abi.FLAG_TOMBSTONE:
                vo = vl = 0
            z.update(val_off=vo if vl else 0, val_len=vl, seq=seq, flags=flags, create_ts=cts, expire_ts=ets)
        return z


# ------------------------------------------------------------------------------------------------
# The reference's own table (tests/golden/get_cases.json, written by tests/golden/make_get_cases.py)
# ------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "get_cases.json")
KEPT_CASES = 23


def golden_cases():
    return json.load(open(GOLDEN))["cases"]


def golden_tree(case, version, block_size=4096, bloom=False):
    """Every layer of a case as a run of one SST, in the order the reference searches them (the fixture's
    layer_order: memtable, immutable memtables, L0 newest first, sorted runs newest first)."""
    runs = []
    for layer in case["layer_order"]:
        es = [(e["key"].encode(), e["kind"], e["value"].encode(), e["seq"], None, e["expire_ts"])
              for e in case["entries"] if e["layer"] == layer]
        runs.append([leaf_of(es, version, block_size, bloom)])
    return Tree(runs)


# ------------------------------------------------------------------------------------------------
# The tree the device tests search
# ------------------------------------------------------------------------------------------------
def _entries(rng, key_ids, seq, merges=True):
    """Sorted entries: 1 to 6 versions per key (values, tombstones, a few merge operands, timestamps), seqs
    descending from `seq`.  Returns (entries, the next free seq below them)."""
    es = []
    for k in sorted(key_ids):
        key = b"k%05d" % k + (b"x" * int(rng.integers(1, 30)) if k % 50 == 0 else b"")
        for _ in range(int(rng.integers(1, 7)) if rng.random() < 0.5 else 1):
            kind = int(rng.choice([0, 0, 0, 2, 2, 1] if merges else [0, 0, 0, 2]))
            es.append((key, kind, bytes(rng.integers(0, 256, int(rng.integers(0, 30)), dtype=np.uint8)), seq,
                       int(rng.integers(0, 2**40)) if rng.random() < 0.2 else None,
                       int(rng.integers(0, 2**40)) if rng.random() < 0.2 else None))
            seq -= 1
    return es, seq


def _cut_inside_key(es, near):
    """An index near `near` with es[i - 1] and es[i] versions of one key (the cut straddles that key)."""
    for i in list(range(near, len(es))) + list(range(near, 0, -1)):
        if 0 < i < len(es) and es[i - 1][0] == es[i][0]:
            return i
    raise AssertionError("no key with several versions")


def _cut_between_keys(es, near):
    i = near
    while es[i - 1][0] == es[i][0]:
        i += 1
    return i


def main_tree(seed=11):
    """4 L0 SSTs and an SST without blocks, then 2 sorted runs of 3 SSTs: block sizes 64 to 256, V1 and V2
    mixed, filters on some SSTs, the newer run cut inside a key's versions, keys >= 400 only in the oldest run.
    Even key numbers exist, odd ones are absent.  Returns (Tree, the key the cut straddles)."""
    rng = np.random.default_rng(seed)
    seq = 10**6
    runs = []
    l0_shape = [(2, 64, True), (1, 128, True), (2, 256, False), (2, 128, True)]
    for j, (version, bs, bloom) in enumerate(l0_shape):
        ids = rng.choice(np.arange(0, 400, 2), 130, replace=False)
        es, seq = _entries(rng, ids, seq)
        runs.append([Leaf(Sst(Batch.from_entries(es), version, bs), bloom)])
        if j == 0:
            runs.append([Leaf(EmptySst())])
    es, seq = _entries(rng, np.arange(0, 400, 2), seq)
    c1, c2 = _cut_inside_key(es, len(es) // 3), _cut_between_keys(es, 2 * len(es) // 3)
    straddler = es[c1][0]
    shape = [(2, 128, True), (1, 64, False), (2, 256, True)]
    runs.append([Leaf(Sst(Batch.from_entries(es[a:b]), v, bs), bl)
                 for (a, b), (v, bs, bl) in zip(((0, c1), (c1, c2), (c2, len(es))), shape)])
    es, seq = _entries(rng, np.arange(0, 520, 2), seq, merges=False)
    c1, c2 = _cut_between_keys(es, len(es) // 3), _cut_between_keys(es, 2 * len(es) // 3)
    shape = [(1, 256, True), (2, 64, True), (2, 128, False)]
    runs.append([Leaf(Sst(Batch.from_entries(es[a:b]), v, bs), bl)
                 for (a, b), (v, bs, bl) in zip(((0, c1), (c1, c2), (c2, len(es))), shape)])
    return Tree(runs), straddler


def main_queries(tree, straddler):
    """About 500 keys: every key number 0..527 (present: even; absent between present ones: odd; present only
    in the oldest run: >= 400; above every last key: > 518), the long-suffix keys, keys below every first key,
    near misses and the straddling key."""
    present = sorted({k for l in tree.leaves for k in l.sst.keys})
    qs = [b"k%05d" % k for k in range(0, 528)] + [k for k in present if len(k) > 6]
    qs += [b"", b"\x00", b"a", b"k", b"zzzz", b"\xff" * 9, straddler, straddler + b"\x00", straddler[:-1]]
    qs += [present[0], present[-1], present[-1] + b"\x00"]
    return qs


def key_seqs(tree, key):
    """Every seq of a key in the tree, newest first."""
    return sorted({r[3] for l in tree.leaves for r in l.sst.rows if r[0] == key}, reverse=True)


def bounded_queries(tree, queries, straddler, seed=3):
    """(keys, max_seq): bounds above all versions, below all, and in the middle of a key's versions; every
    version of the straddling key as a bound, and at it / just under it for every tombstone of 40 keys."""
    rng = np.random.default_rng(seed)
    keys, bounds = [], []
    for q in queries:
        s = key_seqs(tree, q)
        c = int(rng.integers(0, 4))
        b = U64_MAX if c == 0 or not s else (0 if c == 1 else s[int(rng.integers(0, len(s)))] - (c == 3))
        keys.append(q)
        bounds.append(int(b))
    for s in key_seqs(tree, straddler):
        keys += [straddler, straddler]
        bounds += [s, s - 1]
    n = 0
    for l in tree.leaves:
        for r in l.sst.rows:
            if r[4] & _abi.FLAG_TOMBSTONE and n < 80:
                keys += [r[0], r[0]]
                bounds += [r[3], r[3] - 1]
                n += 1
    return keys, bounds
