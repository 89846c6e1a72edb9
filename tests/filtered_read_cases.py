"""Expected results of sdb_lsm_scan_filtered and sdb_lsm_get_filtered: rules F1-F5 of include/slatedb_amd.h restated
literally on top of lsm_scan_cases.scan, get_cases.Tree and the oracle's Filter::might_match (oracle.might_match,
pinned by the reference's filter vectors).
  F1  the query of a (range, SST) pair: a point range (both bounds included, equal keys) asks Point(key), also when
      it has a prefix; else Prefix(p) when it has one; else nothing.  A get always asks Point(key);
  F2  the answer is might_match under the SST's policy; probe_len is what a LENGTHS extractor says (None / -1 /
      beyond the target: None); no bloom: the SST takes part; an empty bitmap answers no to whatever has a probe;
  F3  a ruled-out SST of rule 1 takes no part in the range: no blocks, no candidates, no errors; it is counted in
      range_filtered instead of range_ssts;
  F5  in the get only the filter step of get_cases.Tree.step changes.
"""
import collections

import numpy as np

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd.batch import Batch

from . import get_cases as G
from . import lsm_scan_cases as L
from .scan_cases import EXC, INC, U, Sst

NONE, FIXED, DELIM, LENGTHS = _abi.PREFIX_NONE, _abi.PREFIX_FIXED, _abi.PREFIX_DELIM, _abi.PREFIX_LENGTHS
Policy = collections.namedtuple("Policy", "kind arg no_whole_key")
PLAIN = Policy(NONE, 0, 0)

# L.Scan's fields, and filtered: the SSTs of rule 1 that the filter ruled out
FScan = collections.namedtuple("FScan", L.Scan._fields + ("filtered",))


class Leaf(G.Leaf):
    """An SST with the filter its policy built: bloom None (no filter), an empty array or the bitmap."""

    def __init__(self, sst, policy=PLAIN, bloom=None, num_probes=0, block_status=None, version=None):
        super().__init__(sst, False, block_status, version)
        self.policy, self.bloom, self.num_probes = policy, bloom, num_probes


def build_leaf(entries, version, block_size, policy=PLAIN, bpk=10, lengths=None, bloom="built"):
    """entries sorted as an SST holds them; the filter as the reference's builder makes it for the policy
    (min_filter_keys = 1: always built); lengths: the LENGTHS extractor's answer for every key; bloom: "built",
    None (the view carries no filter) or "empty" (a bitmap of no bytes)."""
    batch = Batch.from_entries(entries)
    if policy.kind == LENGTHS:
        batch.prefix_len = np.full(batch.n, lengths, np.int32)
    enc = O.encode_sst(batch, O.params(block_size=block_size, sst_version=version, bloom_bits_per_key=bpk,
                                       min_filter_keys=1, prefix_kind=policy.kind, prefix_arg=policy.arg,
                                       no_whole_key=policy.no_whole_key))
    assert enc.status == 0 and enc.summary.filter_built
    bm = {"built": enc.bloom, None: None, "empty": np.zeros(0, np.uint8)}[bloom]
    return Leaf(Sst(batch, version, block_size), policy, bm, O.optimal_num_probes(bpk))


def is_point(rng):
    s, sk, e, ek = rng
    return sk == INC and ek == INC and (s or b"") == (e or b"")


def query(rng, prefix):
    """F1 -> (target, is_prefix) or None."""
    if is_point(rng):
        return rng[0] or b"", False
    return None if prefix is None else (prefix, True)


def ruled_out(leaf, q, probe_len=None):
    """F2: the SST's filter answers no."""
    if q is None or leaf.bloom is None or leaf.policy.kind > LENGTHS:
        return False
    target, is_prefix = q
    given = -1 if probe_len is None or probe_len > len(target) else int(probe_len)
    return not O.might_match(leaf.bloom, leaf.num_probes, not leaf.policy.no_whole_key, leaf.policy.kind,
                             leaf.policy.arg, target, is_prefix, given)


class _Hole:
    """What a ruled-out SST is to lsm_scan_cases.scan: an SST without blocks, which takes part in nothing."""
    sst = G.EmptySst()


class _Masked:
    def __init__(self, tree, out):
        self.leaves = [_Hole if i in out else l for i, l in enumerate(tree.leaves)]
        self.block_base = tree.block_base


def scan(tree, rng, prefix=None, probe_len=None, max_seq=None, descending=False):
    """F3: lsm_scan_cases.scan over the tree without the SSTs of rule 1 that the filter rules out for the range."""
    q = query(rng, prefix)
    out = []
    if rng[1] <= EXC and rng[3] <= EXC:
        out = [i for i, l in enumerate(tree.leaves) if L.meets(l, rng) and ruled_out(l, q, probe_len)]
    return FScan(*L.scan(_Masked(tree, set(out)), rng, max_seq, descending), out)


class Tree(G.Tree):
    """get_cases.Tree with rule 2's filter step replaced by F2 for Point(key) (F5)."""
    probe_len = None  # of the key being looked up

    def step(self, i, key):
        l = self.leaves[i]
        if l.policy.kind > LENGTHS:  # checked before the filter
            return _abi.SDB_INVALID_ARGUMENT, (0, 0)
        if ruled_out(l, (key, False), self.probe_len):
            return "filtered", (0, 0)
        saved, l.bloom = l.bloom, None
        try:
            return super().step(i, key)
        finally:
            l.bloom = saved

    def get(self, key, max_seq=None, probe_len=None):
        self.probe_len = probe_len
        try:
            return super().get(key, max_seq)
        finally:
            self.probe_len = None


def honours_f4(tree, rng, prefix):
    """Every key of the range starts with the prefix (over the keys the tree holds)."""
    s, sk, e, ek = L._norm(rng)
    return prefix is None or all(k.startswith(prefix) for k in L.all_keys(tree) if L.contains(k, s, sk, e, ek))


# ------------------------------------------------------------------------------------------------
# The trees the tests read
# ------------------------------------------------------------------------------------------------
TENANTS = 8
SEED = 10


def tenant(t):
    return b"t%02d:" % t


def key(t, x):
    return b"t%02d:%04d" % (t, x)


def prefix_range(p):
    """The range Db::scan_prefix(p, ..) scans: [p, the next prefix)."""
    return (p, INC, p[:-1] + bytes([p[-1] + 1]), EXC)


def _entries(rng, tenants, per_tenant, seq, kinds=(0, 0, 0, 2)):
    """Sorted entries of `per_tenant` keys of each tenant, 1 to 3 versions per key, seqs descending from seq."""
    es = []
    for t in sorted(tenants):
        for x in sorted(rng.choice(100, per_tenant, replace=False).tolist()):
            for _ in range(int(rng.integers(1, 4)) if rng.random() < 0.4 else 1):
                es.append((key(t, x), int(rng.choice(kinds)), bytes(rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8)),
                           seq, int(rng.integers(0, 2**40)) if rng.random() < 0.2 else None,
                           int(rng.integers(0, 2**40)) if rng.random() < 0.2 else None))
                seq -= 1
    return es, seq


L0_TENANTS = ((0, 3, 7), (0, 4, 7), (1, 4, 7))
LENGTHS_LEN = 3  # what the LENGTHS extractor answers: "tNN" of "tNN:xxxx"


def main_tree(seed=SEED):
    """3 L0 SSTs, each holding 3 of the 8 tenants, and one sorted run of 3 SSTs over all tenants, cut inside tenants
    2 and 4; 100 to 200 entries each, block sizes 64 to 256, V1 and V2 mixed.  The filters:
      0  FIXED(4) with whole keys            3  whole keys only (the plain policy)
      1  DELIM(':') without whole keys       4  FIXED(4), no filter in the view (bloom NULL)
      2  LENGTHS with whole keys, at 2 bits  5  an empty bitmap under DELIM(0xFF) without whole keys: no query has
         per key: false positives               anything to probe there"""
    rng = np.random.default_rng(seed)
    seq = 10**6
    shape = [(2, 64, Policy(FIXED, 4, 0), 10), (1, 128, Policy(DELIM, ord(":"), 1), 10), (2, 256, Policy(LENGTHS, 0, 0), 2)]
    runs = []
    for tenants, (version, bs, pol, bpk) in zip(L0_TENANTS, shape):
        es, seq = _entries(rng, tenants, 40, seq)
        runs.append([build_leaf(es, version, bs, pol, bpk, LENGTHS_LEN)])
    es, seq = _entries(rng, range(TENANTS), 35, seq)
    at = lambda k: next(i for i, e in enumerate(es) if e[0] >= k)  # noqa: E731
    c1, c2 = G._cut_between_keys(es, at(key(2, 50))), G._cut_between_keys(es, at(key(4, 50)))
    run_shape = [(2, 128, PLAIN, "built"), (1, 64, Policy(FIXED, 4, 0), None), (2, 256, Policy(DELIM, 0xFF, 1), "empty")]
    runs.append([build_leaf(es[a:b], v, bs, pol, 10, None, bloom)
                 for (a, b), (v, bs, pol, bloom) in zip(((0, c1), (c1, c2), (c2, len(es))), run_shape)])
    return Tree(runs)


def prefix_pairs(tree):
    """(tenant, SST, ruled out, the SST holds a key of the tenant) for every tenant's scan_prefix range and every
    SST of rule 1."""
    out = []
    for t in range(TENANTS):
        p = tenant(t)
        rng = prefix_range(p)
        for i, l in enumerate(tree.leaves):
            if L.meets(l, rng):
                out.append((t, i, ruled_out(l, query(rng, p), LENGTHS_LEN), any(k.startswith(p) for k in l.sst.keys)))
    return out


def uniform_tree(seed=4):
    """Every SST under FIXED(4) without whole keys, the tree the unfiltered get cannot serve: 2 L0 SSTs and a run of
    2; some keys are shorter than the prefix ("t0", "t03": no prefix, so they are always searched)."""
    rng = np.random.default_rng(seed)
    pol = Policy(FIXED, 4, 1)
    seq = 10**5
    runs = []
    for tenants, (version, bs) in zip(((0, 2, 5), (1, 2, 6)), ((2, 64), (1, 128))):
        es, seq = _entries(rng, tenants, 20, seq)
        es = sorted(es + [(b"t0", 0, b"short", seq - 1, None, None), (b"t03", 0, b"short3", seq - 2, None, None)],
                    key=lambda e: (e[0], -e[3]))
        seq -= 3
        runs.append([build_leaf(es, version, bs, pol)])
    es, seq = _entries(rng, (0, 3, 4, 7), 25, seq)
    c = G._cut_between_keys(es, len(es) // 2)
    runs.append([build_leaf(es[:c], 2, 128, pol), build_leaf(es[c:], 1, 64, pol)])
    return Tree(runs)


def scan_cases(tree):
    """(range, prefix or None, probe_len) of every scan case of the device tests; probe_len is what the LENGTHS
    extractor says of the query."""
    keys = L.all_keys(tree)
    out = []
    for t in range(TENANTS):  # every tenant as scan_prefix(p, ..)
        out.append((prefix_range(tenant(t)), tenant(t), LENGTHS_LEN))
    for t in (0, 3, 4, 6):  # sub-ranges inside a tenant
        out.append(((key(t, 10), INC, key(t, 60), EXC), tenant(t), LENGTHS_LEN))
        out.append(((key(t, 30), EXC, key(t, 99), INC), tenant(t), LENGTHS_LEN))
        out.append(((tenant(t), INC, key(t, 20), INC), tenant(t), LENGTHS_LEN))
    out.append((prefix_range(b"t0"), b"t0", -1))  # shorter than FIXED(4), no delimiter, no LENGTHS answer: None everywhere
    out.append((prefix_range(b"t0"), b"t0", LENGTHS_LEN))  # a probe_len beyond the prefix counts as None
    for t in (2, 5, 7):
        out.append((prefix_range(b"t%02d:0" % t), b"t%02d:0" % t, LENGTHS_LEN))  # longer than FIXED(4), bytes after the delimiter
        out.append((prefix_range(b"t%02d" % t), b"t%02d" % t, LENGTHS_LEN))  # no delimiter: None for DELIM, too short for FIXED
    out.append(((None, U, None, U), None, -1))  # has_prefix = 0: no query
    out.append((prefix_range(tenant(3)), None, -1))
    out.append(((key(1, 0), INC, key(5, 0), EXC), None, LENGTHS_LEN))
    present = [keys[len(keys) // 7], keys[len(keys) // 2], keys[-3]]
    for k in present + [key(3, 100), key(6, 7) + b"x", b"t03", b"t0"]:  # point ranges: Point(key) whatever the prefix says
        out.append(((k, INC, k, INC), k[:4], LENGTHS_LEN))
        out.append(((k, INC, k, INC), None, -1))
    out.append(((key(3, 50), INC, key(3, 10), INC), tenant(3), LENGTHS_LEN))  # empty as a set
    out.append(((key(3, 50), EXC, key(3, 50), INC), tenant(3), LENGTHS_LEN))
    return out


def get_keys(tree, seed=6):
    """Every key of the tree, as many absent ones, near misses and keys shorter than the prefix."""
    rng = np.random.default_rng(seed)
    keys = L.all_keys(tree)
    absent = [key(int(rng.integers(0, TENANTS)), int(rng.integers(0, 130))) for _ in range(len(keys))]
    return keys + absent + [b"", b"t0", b"t03", b"t03:", b"t99:0001", keys[5] + b"\x00", keys[9][:-1]]


def merge_tree(seed=8):
    """Operand chains across SSTs under tenant prefixes, as merge_read_cases.chain_tree builds them: 3 L0 SSTs of 3
    tenants each and a run of 2 over all tenants, three entries in five merge operands; every filter FIXED(4) with
    whole keys."""
    rng = np.random.default_rng(seed)
    pol = Policy(FIXED, 4, 0)
    kinds = (1, 1, 1, 0, 2)
    seq = 10**6
    runs = []
    for tenants, (version, bs) in zip(L0_TENANTS, ((2, 64), (1, 128), (2, 256))):
        es, seq = _entries(rng, tenants, 30, seq, kinds)
        runs.append([build_leaf(es, version, bs, pol)])
    es, seq = _entries(rng, range(TENANTS), 25, seq, kinds)
    c = G._cut_inside_key(es, len(es) // 2)
    runs.append([build_leaf(es[:c], 2, 128, pol), build_leaf(es[c:], 1, 64, pol)])
    return Tree(runs)


def mixed_merge_tree(seed=8):
    """merge_tree's chains under main_tree's policies, which do not agree, so a merging get probes per SST: the L0
    SSTs under FIXED(4) with whole keys, DELIM(':') without whole keys and LENGTHS with whole keys; the run's first
    SST under the plain policy, its second without a filter; the run cut inside a key's versions."""
    rng = np.random.default_rng(seed)
    kinds = (1, 1, 1, 0, 2)
    seq = 10**6
    shape = [(2, 64, Policy(FIXED, 4, 0)), (1, 128, Policy(DELIM, ord(":"), 1)), (2, 256, Policy(LENGTHS, 0, 0))]
    runs = []
    for tenants, (version, bs, pol) in zip(L0_TENANTS, shape):
        es, seq = _entries(rng, tenants, 30, seq, kinds)
        runs.append([build_leaf(es, version, bs, pol, 10, LENGTHS_LEN)])
    es, seq = _entries(rng, range(TENANTS), 25, seq, kinds)
    c = G._cut_inside_key(es, len(es) // 2)
    runs.append([build_leaf(es[:c], 2, 128, PLAIN), build_leaf(es[c:], 1, 64, Policy(FIXED, 4, 0), bloom=None)])
    return Tree(runs)
