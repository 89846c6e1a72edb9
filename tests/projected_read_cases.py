"""Expected results of sdb_lsm_scan_projected and sdb_lsm_get_projected: rules P1-P4 of include/slatedb_amd.h
restated literally on top of filtered_read_cases (F1-F5) and lsm_scan_cases.meets.  A visible range is None (the
whole SST) or a range (start, start_kind, end, end_kind) as the scans take them.
  P1  E[i] = [first_key, last_key] intersected with visible[i] (BytesRange::intersect: the tighter start, the tighter
      end, None when empty as a set); an SST with an empty E takes part in nothing;
  P2  SST i is in key k's chain iff E[i] holds k; in a run: a partition point over the effective start keys
      max(first_key, visible start), the last such SST if its E holds k, the SSTs right before it while theirs does;
  P3  per (range, SST) the view range V = range intersected with visible[i]; rules 1-3 with V in place of the range;
  P4  V a point and the range not: the pair asks Point(k) with no probe_len; else the range's own query.
"""
import json
import os

import numpy as np

from slatedb_amd import _abi
from slatedb_amd.batch import Batch

from . import filtered_read_cases as F
from . import get_cases as G
from . import lsm_scan_cases as L
from .scan_cases import EXC, INC, U, Sst, contains, empty_as_set, partitions_covering_range

OPEN = (b"", U, b"", U)


def intersect(a, b):
    """BytesRange::intersect (comparable_range.rs:224-236) of two ranges; None: empty (non_empty, :265-274)."""
    (s1, k1, e1, q1), (s2, k2, e2, q2) = L._norm(a), L._norm(b)
    # starts: Unbounded < Included(a) < Excluded(a); ends: Excluded(a) < Included(a) < Unbounded
    s, sk = max([(s1, k1), (s2, k2)], key=lambda x: (x[1] != U, x[0] if x[1] != U else b"", x[1]))
    e, ek = min([(e1, q1), (e2, q2)], key=lambda x: (x[1] == U, x[0] if x[1] != U else b"", -x[1]))
    return None if empty_as_set(s, sk, e, ek) else (s, sk, e, ek)


def effective(leaf, vis):
    """P1: E of an SST, or None."""
    if not leaf.sst.keys:
        return None
    phys = (leaf.first_key, INC, leaf.last_key, INC)
    return phys if vis is None else intersect(phys, vis)


def holds(rng, key):
    return rng is not None and contains(key, *L._norm(rng))


def view_range(rng, vis):
    """P3: V of a pair, or None."""
    return L._norm(rng) if vis is None else intersect(rng, vis)


def pair_query(rng, V, prefix, probe_len):
    """P4 -> (query, probe_len)."""
    if F.is_point(V) and not F.is_point(rng):
        return (V[0], False), None
    return F.query(rng, prefix), probe_len


def scan(tree, visible, rng, prefix=None, probe_len=None, max_seq=None, descending=False):
    """lsm_scan_cases.scan with every SST's range replaced by its view range, and filtered_read_cases' filter step
    under P4's query -> filtered_read_cases.FScan."""
    s, sk, e, ek = L._norm(rng)
    if sk > EXC or ek > EXC:
        return F.FScan([], _abi.SDB_INVALID_ARGUMENT, [], set(), 0, 0, [])
    bound = L.U64_MAX if max_seq is None else int(max_seq)
    ssts, filtered, status, blocks, cands = [], [], 0, set(), []
    for i, l in enumerate(tree.leaves):  # search order
        V = view_range(rng, visible[i])
        if V is None or not L.meets(l, V):
            continue
        q, pl = pair_query(rng, V, prefix, probe_len)
        if F.ruled_out(l, q, pl):
            filtered.append(i)
            continue
        ssts.append(i)
        base = int(tree.block_base[i])
        if l.version not in (1, 2):
            status = status or _abi.SDB_INVALID_VERSION
            continue
        bs, be = partitions_covering_range(l.sst.index_keys, *V)
        be = max(be, bs)
        blocks |= {base + b for b in range(bs, be)}
        for b in range(bs, be):
            if l.block_status.get(b) and not status:
                status = l.block_status[b]
        cands += [(i, x) for x in range(l.sst.bes[bs], l.sst.bes[be]) if contains(l.sst.keys[x], *V)]
    if status:
        return F.FScan([], status, ssts, blocks, 0, 0, filtered)
    ckb = sum(len(tree.leaves[i].sst.keys[x]) for i, x in cands)
    order = sorted((tree.leaves[i].sst.keys[x], -tree.leaves[i].sst.rows[x][3], i, x) for i, x in cands
                   if tree.leaves[i].sst.rows[x][3] <= bound)
    rows, last = [], None
    for key, _, i, x in order:
        if key == last:
            continue
        last = key
        flags = tree.leaves[i].sst.rows[x][4]
        if flags & _abi.FLAG_TOMBSTONE:
            continue
        if flags & _abi.FLAG_MERGE_OPERAND:
            return F.FScan([], _abi.SDB_MERGE_OPERATOR_MISSING, ssts, blocks, len(cands), ckb, filtered)
        rows.append((key, i, x))
    if descending:
        rows.reverse()
    return F.FScan(rows, 0, ssts, blocks, len(cands), ckb, filtered)


class Tree(F.Tree):
    """filtered_read_cases.Tree with rule 1's chain replaced by P2."""

    def __init__(self, runs, visible):
        super().__init__(runs)
        assert len(visible) == len(self.leaves)
        self.visible = list(visible)

    def eff_start_le(self, i, key):
        """compacted_effective_start_key of SST i is <= key."""
        l, vis = self.leaves[i], self.visible[i]
        if not l.sst.keys or l.first_key > key:
            return False
        return vis is None or vis[1] == U or (vis[0] or b"") <= key

    def in_chain(self, i, key):
        return holds(effective(self.leaves[i], self.visible[i]), key)

    def chain(self, key):
        out, i0 = [], 0
        for run in self.runs:
            lo, hi = i0, i0 + len(run)  # partition_point(effective start <= key)
            while lo < hi:
                mid = lo + (hi - lo) // 2
                if self.eff_start_le(mid, key):
                    lo = mid + 1
                else:
                    hi = mid
            if lo > i0 and self.in_chain(lo - 1, key):
                first = lo - 1
                while first > i0 and self.in_chain(first - 1, key):
                    first -= 1
                out += list(range(first, lo))
            i0 += len(run)
        return out


def projected(tree, visible):
    """A filtered_read_cases / get_cases tree under projections."""
    it = iter([l if isinstance(l, F.Leaf) else F.Leaf(l.sst, F.PLAIN, l.bloom, G.NUM_PROBES, l.block_status, l.version)
               for l in tree.leaves])  # a get_cases leaf: its whole-key filter under the plain policy
    return Tree([[next(it) for _ in r] for r in tree.runs], visible)


# ------------------------------------------------------------------------------------------------
# The second oracle: every projected SST physically trimmed to its visible rows, read without projections
# ------------------------------------------------------------------------------------------------
def entries_of(leaf, keep):
    """(key, kind, value, seq, create_ts, expire_ts) of the rows of an SST that `keep` takes."""
    out = []
    for key, vo, vl, seq, flags, cts, ets in leaf.sst.rows:
        if keep(key):
            kind = 2 if flags & _abi.FLAG_TOMBSTONE else (1 if flags & _abi.FLAG_MERGE_OPERAND else 0)
            out.append((key, kind, leaf.sst.data[vo:vo + vl].tobytes(), seq, cts, ets))
    return out


def trimmed(tree, visible, block_size=128):
    """The tree with SST i holding only the rows its visible range contains (an SST without such rows becomes
    get_cases.EmptySst), no filters: a get_cases.Tree for the unprojected models."""
    leaves = []
    for l, vis in zip(tree.leaves, visible):
        if vis is None or not l.sst.keys:
            leaves.append(G.Leaf(l.sst, False, None, l.version))
            continue
        es = entries_of(l, lambda k: contains(k, *L._norm(vis)))
        leaves.append(G.Leaf(Sst(Batch.from_entries(es), l.sst.version, block_size) if es else G.EmptySst()))
    it = iter(leaves)
    return G.Tree([[next(it) for _ in r] for r in tree.runs])


def row_value(tree, i, x):
    """(key, seq, flags, value bytes) of row x of SST i."""
    l = tree.leaves[i]
    key, vo, vl, seq, flags = l.sst.rows[x][:5]
    return key, seq, flags, l.sst.data[vo:vo + vl].tobytes()


# ------------------------------------------------------------------------------------------------
# Random projections (the CPU sweep and the device tests read the same seeded cases)
# ------------------------------------------------------------------------------------------------
def bound_keys(leaf, rng):
    """What a visible bound of an SST is drawn from: present keys, absent keys, one byte past a key, prefixes of
    keys, and keys before the first and after the last."""
    ks = leaf.sst.keys
    k = ks[int(rng.integers(0, len(ks)))]
    c = int(rng.integers(0, 8))
    if c < 3:
        return k
    if c == 3:
        return k[:-1] + bytes([min(k[-1] + 1, 255)]) + b"~"  # absent, above k
    if c == 4:
        return k + b"\x00"
    if c == 5:
        return k[:max(1, len(k) - 2)]
    return leaf.first_key[:1] if c == 6 else leaf.last_key + b"\xff"


def random_projections(tree, seed, open_share=0.25):
    """One visible range or None per SST: the start Unbounded or Included, the end any kind; mostly start <= end."""
    rng = np.random.default_rng(seed)
    out = []
    for l in tree.leaves:
        if not l.sst.keys or rng.random() < open_share:
            out.append(None)
            continue
        a, b = bound_keys(l, rng), bound_keys(l, rng)
        if a > b and rng.random() < 0.9:
            a, b = b, a
        sk = INC if rng.random() < 0.8 else U
        ek = (INC, EXC, U)[int(rng.choice(3, p=[0.4, 0.4, 0.2]))]
        out.append((a if sk else None, sk, b if ek else None, ek))
    return out


def sweep_stats(tree, visible, cases):
    """Over the (range, SST) pairs that take part unprojected: how many still take part, and how many lose at least
    one candidate to the projection."""
    pairs = still = lose = 0
    for rng, prefix, pl in cases:
        free = F.scan(tree, rng, prefix, pl)
        if free.status or rng[1] > EXC or rng[3] > EXC:
            continue
        proj = scan(tree, visible, rng, prefix, pl)
        for i in free.ssts:
            pairs += 1
            still += i in proj.ssts
            l = tree.leaves[i]
            n_free = sum(contains(k, *L._norm(rng)) for k in l.sst.keys)
            V = view_range(rng, visible[i])
            n_proj = sum(contains(k, *V) for k in l.sst.keys) if V is not None and i in proj.ssts else 0
            lose += n_proj < n_free
    return pairs, still, lose


def point_tree(seed=2):
    """Three L0 SSTs over tenants 0 to 2 with the same key span: FIXED(4) with whole keys, LENGTHS without whole keys
    (a point that is one only through a projection has no length there: None) and DELIM(':') without whole keys.
    Returns (Tree's runs as filtered_read_cases.Tree, a key of tenant 1 that every SST holds, one that none holds)."""
    rng = np.random.default_rng(seed)
    seq, runs = 10**5, []
    shape = [(2, 64, F.Policy(F.FIXED, 4, 0)), (1, 128, F.Policy(F.LENGTHS, 0, 1)), (2, 128, F.Policy(F.DELIM, ord(":"), 1))]
    for version, bs, pol in shape:
        es, seq = F._entries(rng, (0, 1, 2), 30, seq)
        es = sorted(es + [(F.key(1, 500), 0, b"here", seq - 1, None, None)], key=lambda e: (e[0], -e[3]))
        seq -= 2
        runs.append([F.build_leaf(es, version, bs, pol, 10, F.LENGTHS_LEN)])
    return F.Tree(runs), F.key(1, 500), F.key(1, 501)


LONG = b"e060"  # the key of edge_tree whose versions fill more than three blocks


def edge_tree(seed=7, block_size=96):
    """Twelve L0 SSTs over the same entries, six V2 and six V1: 60 keys of one version and LONG with 40.  Every SST
    of a version gets one of six visible bounds (edge_projections), so one call reads every position of a bound."""
    rng = np.random.default_rng(seed)
    es, seq = [], 10**4
    for x in range(0, 120, 2):
        for _ in range(40 if b"e%03d" % x == LONG else 1):
            es.append((b"e%03d" % x, int(rng.choice((0, 0, 0, 2))), bytes(rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8)),
                       seq, None, int(rng.integers(0, 2**40)) if rng.random() < 0.2 else None))
            seq -= 1
    base = [F.build_leaf(es, v, block_size, bloom=None) for v in (2, 1)]
    return F.Tree([[F.Leaf(b.sst, b.policy, None, 0)] for b in base for _ in range(6)])


def edge_keys(leaf):
    """(a block's index key, a key in the middle of a block, an absent key between two blocks) of an SST, away from
    LONG's blocks."""
    s = leaf.sst
    b = next(b for b in range(1, s.nb - 1) if s.bes[b + 1] - s.bes[b] >= 3 and s.keys[s.bes[b + 1]] < LONG)
    gap = s.keys[s.bes[b + 1] - 1] + b"\x00"
    # (a V2 index key is a shortened separator: above the block before, at most the block's first key)
    assert s.keys[s.bes[b] - 1] < s.index_keys[b] <= s.keys[s.bes[b]] and gap not in s.keys and gap < s.keys[s.bes[b + 1]]
    return s.index_keys[b], s.keys[s.bes[b] + 1], gap


def edge_projections(tree, side):
    """Per SST, where its visible start (side "start") or end ("end") falls: on a block's index key, mid-block, on
    an absent key between two blocks, outside the physical range (visible wider than the SST), and on LONG:
    included, and then excluded (as an end) or just behind it (as a start: a start is never excluded)."""
    out = []
    for j, l in enumerate(tree.leaves):
        ik, mid, gap = edge_keys(l)
        if side == "start":
            out.append([(ik, INC, None, U), (mid, INC, None, U), (gap, INC, None, U), (b"a", INC, b"z", INC),
                        (LONG, INC, None, U), (LONG + b"\x00", INC, None, U)][j % 6])
        else:
            out.append([(None, U, ik, EXC), (None, U, mid, INC), (None, U, gap, EXC), (None, U, ik, INC),
                        (None, U, LONG, INC), (None, U, LONG, EXC)][j % 6])
    return out


def edge_ranges(tree):
    keys = L.all_keys(tree)
    out = [(None, U, None, U), (LONG, INC, None, U), (LONG, EXC, None, U), (None, U, LONG, EXC), (None, U, LONG, INC)]
    marks = [LONG] + [k for l in (tree.leaves[0], tree.leaves[6]) for k in edge_keys(l)]
    for k in marks:
        out.append((k, INC, k, INC))
        j = min(range(len(keys)), key=lambda x: (keys[x] < k, keys[x]))  # the first key >= k
        lo, hi = keys[max(0, j - 2)], keys[min(len(keys) - 1, j + 2)]
        out += [(lo, sk, hi, ek) for sk in (INC, EXC) for ek in (INC, EXC)] + [(k, INC, hi, EXC), (lo, EXC, k, INC)]
    return out


def long_seqs(tree):
    return sorted(r[3] for r in tree.leaves[0].sst.rows if r[0] == LONG)


def straddle_run(seed=3):
    """One sorted run of three SSTs, cut inside a key's versions and then between keys; the left SST's view ends,
    excluded, at the straddling key, so only the right one holds it.  -> (tree, visible, the key)."""
    rng = np.random.default_rng(seed)
    es, _ = F._entries(rng, (0, 1, 2), 40, 10**5)
    c1, c2 = G._cut_inside_key(es, len(es) // 3), G._cut_between_keys(es, 2 * len(es) // 3)
    k = es[c1][0]
    run = [F.build_leaf(es[a:b], v, bs) for (a, b), (v, bs) in zip(((0, c1), (c1, c2), (c2, len(es))), ((2, 64), (1, 128), (2, 64)))]
    return F.Tree([run]), [(None, U, k, EXC), None, None], k


def key_gap_run(case):
    """The fixture's run [a, c] and [m, p] projected to a case's global range -> (tree, visible)."""
    g = golden()["key_gap"]
    keys = {"a": [b"a", b"b", b"c"], "m": [b"m", b"n", b"p"]}
    run = [F.build_leaf([(k, 0, b"value", 7, None, None) for k in keys[s["first"]]], 2, 64) for s in g["run"]]
    glob = golden_range(case["global_range"])
    return F.Tree([run]), [intersect(golden_range(s["visible"]), glob) or glob for s in g["run"]]


K1, K2 = b"x030", b"x035"


def hidden_l0():
    """Two L0 SSTs with overlapping physical ranges and disjoint views.  The newer one holds, outside its view, a
    newer value over a tombstone for K1 and a newer operand for K2; the older one holds K1's value and K2's operand
    chain with its base.  -> (tree, visible)."""
    e = lambda k, kind, v, seq: (k, kind, v, seq, None, None)  # noqa: E731
    newer = [e(b"x0%02d" % i, 0, b"n%d" % i, 300 + i) for i in range(10, 50, 5) if i not in (30, 35)]
    newer += [e(K1, 0, b"newer", 250), e(K1, 2, b"", 240), e(K2, 1, b"hidden-op", 245)]
    older = [e(b"x0%02d" % i, 0, b"o%d" % i, 100 + i) for i in range(20, 60, 5) if i not in (30, 35)]
    older += [e(K1, 0, b"old", 70), e(K2, 1, b"op2", 90), e(K2, 1, b"op1", 80), e(K2, 0, b"base", 60)]
    srt = lambda es: sorted(es, key=lambda x: (x[0], -x[3]))  # noqa: E731
    tree = F.Tree([[F.build_leaf(srt(newer), 2, 64)], [F.build_leaf(srt(older), 1, 64)]])
    return tree, [(b"x010", INC, K1, EXC), (K1, INC, None, U)]


class ViewLeaf(F.Leaf):
    """A leaf that covers what its effective range holds: merge_read_cases.get_merge over projections."""

    def covers(self, key):
        return holds(self.E, key)


def merge_view(tree, visible):
    leaves = []
    for l, v in zip(tree.leaves, visible):
        leaves.append(ViewLeaf(l.sst, l.policy, l.bloom, l.num_probes, l.block_status, l.version))
        leaves[-1].E = effective(l, v)
    it = iter(leaves)
    return F.Tree([[next(it) for _ in r] for r in tree.runs])


# seeds under which the model keeps at least half of filtered_read_cases.main_tree's pairs and at least a quarter
# lose a candidate (test_projected_read_cases asserts both; most seeds do, these with a wide margin)
SWEEP_SEEDS = (21, 24, 36)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "projection_cases.json")


def golden():
    return json.load(open(GOLDEN))


def golden_range(r):
    (s, sk), (e, ek) = r
    return (s.encode(), sk, e.encode(), ek)
