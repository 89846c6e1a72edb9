"""Hand-shaped runs for the merge kernels of sdb_compact.hip (k_mg_lcp0, k_mg_prefix, k_mg_bounds, k_mg_rank,
k_mg_keys, k_mg_scan, k_mg_emit), with a plain-Python restatement of what the device decides for them
(`restate`), so that every case can prove on the CPU that it sits on the clause it names.  Five families:

  K  key order: the shared prefix L0 and the 8-byte windows behind it, keys that tie on the window, proper
     prefixes, zero tails, high bytes, an outlier that collapses L0, empty runs, every load8 residue, and
     run-order violations that show only after byte 8;
  R  k_mg_rank's LDS windows on either side of the 2048-prefix limit, mixed LDS / HBM placement, equal
     windows inside an LDS window, 32 runs (sparse: workgroups spanning runs; dense: one run per workgroup);
  V  one hot key whose version walk starts at, ends at or crosses a wave, workgroup or tile boundary, under
     each retention rule;
  S  tile counts around 1024 entries, more than 512 tiles (k_mg_scan's second pass), output capacities;
  C  key and value lengths around the 16-byte chunk and the 128-byte copy step, arranged per 64-entry copy
     group of k_mg_emit; value sources at every residue mod 16; tombstones that carry ignored bytes.

Runs are built from explicit arrays (`make_run`): a tombstone may keep value bytes and a non-zero val_len, and
both arenas may start with filler.  A case is a `Case`: a name, the clauses it aims at, a builder of
(runs, retention) and what it expects."""
import bisect
import functools
import struct

import numpy as np

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd.batch import Run

# sdb_compact.hip / sdb_compact.h
K_PFX_THREADS = 256            # kPfxThreads: global entries (k_mg_prefix, k_mg_rank) / positions (k_mg_keys) per workgroup
K_RANK_LDS_PREFIXES = 2048     # kRankLds / 8: window prefixes a k_mg_rank workgroup stages in LDS
K_MERGE_TILE = 1024            # kMergeTile: merged positions per k_mg_emit workgroup
K_MERGE_THREADS = 512          # kMergeThreads: tiles k_mg_scan takes per pass
K_COPY_STEP = 128              # bytes of one entry a copy step moves (eight lanes of ...
K_CHUNK = 16                   # ... one 16-byte chunk each): the literals 128 and 16 of k_mg_emit / chunk_put
K_COPY_GROUP = (K_MERGE_TILE // 2) // (K_MERGE_THREADS // 64)  # kPerWave: entries a wave copies per half tile
assert K_COPY_GROUP == 64

V, M, T = _abi.KIND_VALUE, _abi.KIND_MERGE, _abi.KIND_TOMBSTONE
KEEP_ALL = dict(time_seq=0)    # every seq inside the time window: no version is dropped for its age


def _pat(n, salt=0):
    """n deterministic bytes."""
    return ((np.arange(n, dtype=np.uint32) * 131 + salt * 29 + 7) % 251).astype(np.uint8).tobytes()


def be32(x):
    return struct.pack(">I", x)


def be64(x):
    return struct.pack(">Q", x)


# ------------------------------------------------------------------------------------------------
# runs from explicit arrays
# ------------------------------------------------------------------------------------------------
def make_run(rows, k0=0, v0=0):
    """rows: (key, kind, value, seq[, create_ts, expire_ts]), sorted by the caller.  A tombstone KEEPS its
    value bytes and their length in val_len; key_off[0] = k0 and the first value starts at v0 (the bytes in
    front are filler).  Values are contiguous, so the run is also a batch."""
    n = len(rows)
    keys = [bytes(r[0]) for r in rows]
    vals = [bytes(r[2]) for r in rows]
    if not n:
        k0 = v0 = 0
    key_off = np.full(n + 1, k0, np.uint64)
    vlen = np.array([len(v) for v in vals], np.uint32)
    val_off = np.full(n, v0, np.uint64)
    if n:
        key_off[1:] += np.cumsum([len(k) for k in keys], dtype=np.uint64)
        val_off[1:] += np.cumsum(vlen[:-1], dtype=np.uint64)
    ts = lambda r, i: r[i] if len(r) > i and r[i] is not None else None
    flags = np.array([(r[1] == T) * _abi.FLAG_TOMBSTONE | (r[1] == M) * _abi.FLAG_MERGE_OPERAND |
                      (ts(r, 4) is not None) * _abi.FLAG_HAS_CREATE_TS | (ts(r, 5) is not None) * _abi.FLAG_HAS_EXPIRE_TS
                      for r in rows], np.uint8)
    return Run(np.frombuffer(b"\xEE" * k0 + b"".join(keys), np.uint8).copy(), key_off,
               np.frombuffer(b"\xDD" * v0 + b"".join(vals), np.uint8).copy(), val_off, vlen,
               np.array([r[3] for r in rows], np.uint64), flags,
               np.array([ts(r, 4) or 0 for r in rows], np.int64), np.array([ts(r, 5) or 0 for r in rows], np.int64))


def keys_of(run):
    ko, a = run.key_off.tolist(), run.key_arena.tobytes()
    return [a[ko[i]:ko[i + 1]] for i in range(run.n)]


def entries_of_run(run):
    """The run as Batch.from_entries rows (a tombstone's ignored bytes dropped): what py_merge takes."""
    ks, vb = keys_of(run), run.val_base.tobytes()
    out = []
    for i, k in enumerate(ks):
        f = int(run.flags[i])
        kind = T if f & _abi.FLAG_TOMBSTONE else M if f & _abi.FLAG_MERGE_OPERAND else V
        o = int(run.val_off[i])
        out.append((k, kind, b"" if kind == T else vb[o:o + int(run.val_len[i])], int(run.seq[i]),
                    int(run.create_ts[i]) if f & _abi.FLAG_HAS_CREATE_TS else None,
                    int(run.expire_ts[i]) if f & _abi.FLAG_HAS_EXPIRE_TS else None))
    return out


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def lcp(a, b):
    m = min(len(a), len(b))
    j = 0
    while j < m and a[j] == b[j]:
        j += 1
    return j


def lcp0(keys):
    """k_mg_lcp0: the prefix run 0's first key (the first non-empty run's) shares with every run's first and last key."""
    e0, L = None, 0
    for ks in keys:
        if not ks:
            continue
        if e0 is None:
            e0, L = ks[0], len(ks[0])
        L = min(L, lcp(e0, ks[0]), lcp(e0, ks[-1]))
    return L


def window(key, L0):
    """k_mg_prefix: key bytes [L0, L0 + 8), big-endian, zero padded."""
    return int.from_bytes(key[L0:L0 + 8].ljust(8, b"\0"), "big")


class State:
    """What the device decides for (runs, retention).  error: the lowest global entry that breaks its run's
    order, or None; the rank, walk and copy facts exist only for sorted runs (the kernels stop at an error)."""


def restate(runs, ret, full=True):
    st = State()
    st.keys = [keys_of(r) for r in runs]
    st.nruns = len(runs)
    st.bases = np.concatenate([[0], np.cumsum([r.n for r in runs])]).astype(np.int64).tolist()
    st.total = st.bases[-1]
    st.L0 = lcp0(st.keys)
    st.win = np.array([window(k, st.L0) if len(k) >= st.L0 else 0 for ks in st.keys for k in ks], np.uint64)
    st.ntiles = (st.total + K_MERGE_TILE - 1) // K_MERGE_TILE
    srt = [list(zip(ks, (-r.seq.astype(object)).tolist())) for ks, r in zip(st.keys, runs)]  # (key asc, seq desc)
    st.error = None
    for r, t in enumerate(srt):
        bad = next((i for i in range(1, len(t)) if t[i - 1] > t[i]), None)
        if bad is not None:
            st.error = st.bases[r] + bad
            break
    if st.error is not None:
        return st
    run_of = lambda g: bisect.bisect_right(st.bases, g, 1, st.nruns) - 1  # empty runs share their successor's base

    def before(r2, r, t):  # entries of run r2 that come before (t, run r): MergeIterator order, run order on ties
        return (bisect.bisect_right if r2 < r else bisect.bisect_left)(srt[r2], t)

    # k_mg_bounds / k_mg_rank, per workgroup of 256 global entries
    gb = (st.total + K_PFX_THREADS - 1) // K_PFX_THREADS
    st.bound = np.zeros((gb, 2, st.nruns), np.uint64)
    st.groups = []
    for b in range(gb):
        g0 = b * K_PFX_THREADS
        gl = min(g0 + K_PFX_THREADS, st.total) - 1
        for side, g in enumerate((g0, gl)):
            r = run_of(g)
            for r2 in range(st.nruns):
                if r2 != r:
                    st.bound[b, side, r2] = before(r2, r, srt[r][g - st.bases[r]])
        r = run_of(g0)
        grp = dict(run=r, one_run=run_of(gl) == r, spans=run_of(gl) - r + 1, win={}, lds={})
        if grp["one_run"]:
            off = 0
            for r2 in range(st.nruns):  # the packing loop: a window that does not fit is left out, later ones still pack
                if r2 == r:
                    continue
                c = int(st.bound[b, 1, r2] - st.bound[b, 0, r2])
                grp["win"][r2] = c
                grp["lds"][r2] = off + c <= K_RANK_LDS_PREFIXES
                if grp["lds"][r2]:
                    off += c
        st.groups.append(grp)
    if not full:
        return st
    # the merged order, the retention decision of every position and the walks of keys with several versions
    order = sorted((t[0], t[1], r, i) for r in range(st.nruns) for i, t in enumerate(srt[r]))
    st.order = [(r, i) for _, _, r, i in order]
    n = st.total
    dec = [0] * n
    st.walks = []
    st.expired_values = st.expired_merges = 0
    cst = ret.compaction_start_ts
    g = 0
    while g < n:
        ge = g + 1
        while ge < n and order[ge][0] == order[g][0]:
            ge += 1
        for q in range(g, ge):
            r, i = st.order[q]
            seq, f = -order[q][1], int(runs[r].flags[i])
            if q + 1 < ge and order[q + 1][1] == order[q][1]:  # a later version with the same seq replaces this one
                continue
            merge = bool(f & _abi.FLAG_MERGE_OPERAND)
            expired = bool(f & _abi.FLAG_HAS_EXPIRE_TS) and int(runs[r].expire_ts[i]) <= cst
            if expired and merge:
                st.expired_merges += 1
                continue
            st.expired_values += expired
            dec[q] = 2 if expired else 1
            if not ((ret.has_time_window and seq >= ret.time_seq) or (ret.has_min_seq and seq > ret.min_seq) or merge):
                break
        if ret.filter_tombstone:
            for q in range(ge - 1, g - 1, -1):
                if not dec[q]:
                    continue
                r, i = st.order[q]
                if dec[q] == 2 or int(runs[r].flags[i]) & _abi.FLAG_TOMBSTONE:
                    dec[q] = 0
                else:
                    break
        if ge - g > 1:
            seqs = [order[q][1] for q in range(g, ge)]
            st.walks.append(dict(p=g, nv=ge - g, dec=dec[g:ge], equal_seqs=len(seqs) - len(set(seqs)),
                                 tiles=sorted({q // K_MERGE_TILE for q in range(g, ge) if dec[q]})))
        g = ge
    st.dec = dec
    # k_mg_emit: what every position copies, and the 64-entry copy groups of each half tile
    kb, vb = [0] * n, [0] * n
    for q, (r, i) in enumerate(st.order):
        if dec[q]:
            kb[q] = len(st.keys[r][i])
            vb[q] = int(runs[r].val_len[i]) if dec[q] == 1 and not int(runs[r].flags[i]) & _abi.FLAG_TOMBSTONE else 0
    st.kb, st.vb = kb, vb
    st.copy = []
    steps = lambda lo, hi: len(range(lo, hi, K_COPY_STEP))
    for s in range(0, n, K_COPY_GROUP):  # tile s / 1024, half (s / 512) % 2, wave w = (s / 64) % 8: positions s .. s + 63
        mk, mv = max(kb[s:s + K_COPY_GROUP]), max(vb[s:s + K_COPY_GROUP])
        joint = steps(0, min(mk, mv))
        st.copy.append(dict(start=s, mk=mk, mv=mv, joint=joint, key_steps=steps(joint * K_COPY_STEP, mk),
                            val_steps=steps(joint * K_COPY_STEP, mv)))
    return st


class Case:
    def __init__(self, name, clauses, build, big=False, **expect):
        self.name, self.clauses, self._build, self.big, self.expect = name, tuple(clauses), build, big, expect

    def __repr__(self):
        return "Case(%s)" % self.name

    @functools.cached_property
    def built(self):
        runs, ret = self._build()
        return runs, O.retention(**ret)

    @property
    def runs(self):
        return self.built[0]

    @property
    def ret(self):
        return self.built[1]

    @functools.cached_property
    def state(self):
        return restate(self.runs, self.ret, full=not self.big)

    @functools.cached_property
    def ref(self):
        return O.merge_runs(self.runs, self.ret)


def _split(rows, nruns):
    """rows: (run, row) pairs in any order -> one make_run per run, each sorted by key asc, seq desc."""
    out = [[] for _ in range(nruns)]
    for r, row in rows:
        out[r].append(row)
    return [sorted(x, key=lambda e: (e[0], -e[3])) for x in out]


# ------------------------------------------------------------------------------------------------
# K: key order
# ------------------------------------------------------------------------------------------------
K_L0S = (0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 1000)
K_DIFF_AT = (8, 15, 16, 17, 200)   # suffixes equal over the whole window that first differ at byte L0 + this
K_ZERO_STEMS = (b"", b"z", b"ZZZZZZZ", b"ZZZZZZZZ")  # k, k + \0, ... k + nine \0: inside, across and past the window
K_HIGH = (0x7F, 0x80, 0xFF)


def k_suffixes():
    s = {b""}
    s |= {b"m" * n for n in range(1, 10)} | {b"m" * 40}  # lengths 1 .. 9 and longer; each a proper prefix of the next
    s |= {bytes([0x30 + n]) * n for n in range(1, 10)}
    for d in K_DIFF_AT:
        s |= {b"TTTTTTTT" + b"f" * (d - 8) + c for c in (b"a", b"b")}
    for stem in K_ZERO_STEMS:
        s |= {stem + b"\0" * j for j in range(10)}
    for b in K_HIGH:
        s |= {bytes([b]), bytes([b]) + b"-thirteen-by", bytes([b]) * 8 + b"x"}
    return sorted(s)


def k_rows(prefix, suffixes, nruns):
    """One version of every key in run i % nruns; every fourth key has an older version in the next run and
    every seventh a version of the same seq in the run after that."""
    rows = []
    for i, s in enumerate(suffixes):
        k = prefix + s
        rows.append((i % nruns, (k, T if i % 11 == 5 else V, _pat(i % 23, i), 1000 + i, i if i % 3 else None, None)))
        if nruns > 1 and i % 4 == 1:
            rows.append(((i + 1) % nruns, (k, V, _pat(i % 19, i + 1), 500 + i)))
        if nruns > 2 and i % 7 == 2:
            rows.append(((i + 2) % nruns, (k, V, _pat(i % 17, i + 2), 1000 + i)))
    return rows


def k_prefix(L0):
    return _pat(L0, 3)


def _k_build(L0, nruns=3, drop_empty_suffix=False):
    def build():
        suf = [s for s in k_suffixes() if s or not drop_empty_suffix]
        return [make_run(r) for r in _split(k_rows(k_prefix(L0), suf, nruns), nruns)], KEEP_ALL
    return build


def _k_outlier():
    rows = k_rows(k_prefix(40), k_suffixes(), 2)
    rows.append((2, (k_prefix(40) + b"mm", V, b"v", 7)))
    rows.append((2, (b"\xff", V, b"outlier", 8)))
    return [make_run(r) for r in _split(rows, 3)], KEEP_ALL


def _k_empty_runs():
    a, b, c = [make_run(r) for r in _split(k_rows(k_prefix(9), k_suffixes(), 3), 3)]
    e = make_run([])
    return [a, e, b, c, e], KEEP_ALL


K_RES_K0 = (0, 3, 5)


def _k_residues():
    """19-byte keys (3 shared bytes, a window one of three values, an 8-byte counter) behind 0, 3 and 5 filler
    bytes: the key starts, the window starts and the bytes compared after a tied window each visit every
    address residue mod 8."""
    rows = []
    for i in range(120):
        rows.append((i % 3, (b"res" + b"%d-WINDOW" % (i // 40) + be64(i), V, _pat(i % 9, i), 300 - i)))
    return [make_run(r, k0=k0) for r, k0 in zip(_split(rows, 3), K_RES_K0)], KEEP_ALL


def _plain_run(tag, n, seq0=10 ** 6):
    return [(tag + b"%06d" % i, V, _pat(i % 7, i), seq0 - i) for i in range(n)]


def _k_err_desc(equal):
    """Run 1: keys equal in their first `equal` bytes, entries 30 and 31 swapped (descending after that)."""
    def build():
        rows = [(b"E" * equal + b"%04d" % i, V, b"v", 500 - i) for i in range(60)]
        rows[30], rows[31] = rows[31], rows[30]
        return [make_run(_plain_run(b"A", 50)), make_run(rows)], KEEP_ALL
    return build


def _k_err_seq():
    """Run 1: 300 versions of one 20-byte key, seqs descending except a step up at entry 200."""
    rows = [(b"one-long-equal-key--", V, b"v", 5000 - i) for i in range(300)]
    rows[200] = rows[200][:3] + (5000 - 198,)
    return [make_run(_plain_run(b"A", 50)), make_run(rows)], KEEP_ALL


def _k_err_two(first_run_clean):
    """Two violations, each after byte 8, in different k_mg_prefix workgroups."""
    def build():
        def run(bad):
            rows = [(b"SAMEFIRST8" + b"%05d" % i, V, b"v", 9000 - i) for i in range(600)]
            for i in bad:
                rows[i - 1], rows[i] = rows[i], rows[i - 1]
            return make_run(rows)
        if first_run_clean:
            return [run(()), run((100, 500))], KEEP_ALL     # global entries 700 and 1100
        return [run((500,)), run((300,))], KEEP_ALL         # global entries 500 and 900
    return build


def k_cases():
    out = []
    shapes = ("lcp0", "short-keys", "window-ties", "prefix-keys", "zero-tails", "high-bytes")
    for L0 in K_L0S:
        out.append(Case("K/L0-%d" % L0, shapes + (("empty-first-key",) if L0 == 0 else ()), _k_build(L0), L0=L0))
    out.append(Case("K/L0-9-no-key-of-length-L0", ("lcp0", "window-ties", "prefix-keys", "high-bytes"), _k_build(9, drop_empty_suffix=True), L0=9))
    out.append(Case("K/L0-16-two-runs", shapes, _k_build(16, nruns=2), L0=16))
    out.append(Case("K/L0-17-four-runs", shapes, _k_build(17, nruns=4), L0=17))
    out.append(Case("K/outlier", ("lcp0", "outlier"), _k_outlier, L0=0))
    out.append(Case("K/empty-runs", ("lcp0", "empty-run"), _k_empty_runs, L0=9))
    out.append(Case("K/residues", ("lcp0", "load8-residues", "window-ties"), _k_residues, L0=3))
    INV = _abi.SDB_INVALID_ARGUMENT
    out.append(Case("K/err-desc-after-8", ("order-after-8",), _k_err_desc(8), status=INV, entry=81, equal=8))
    out.append(Case("K/err-desc-after-16", ("order-after-8",), _k_err_desc(16), status=INV, entry=81, equal=16))
    out.append(Case("K/err-seq-ascending", ("order-seq",), _k_err_seq, status=INV, entry=250))
    out.append(Case("K/err-two-runs", ("order-two",), _k_err_two(False), status=INV, entry=500, all_errors=(500, 900)))
    out.append(Case("K/err-two-workgroups", ("order-two",), _k_err_two(True), status=INV, entry=700,
                    all_errors=(700, 1100)))
    return out


def k_many_runs():
    """L0 > 0 over 35 runs: the compactor merges groups of 32 first, each raw merge with an L0 of its own."""
    return Case("K/L0-16-35-runs", ("lcp0",), _k_build(16, nruns=35), L0=16)


# ------------------------------------------------------------------------------------------------
# R: rank windows
# ------------------------------------------------------------------------------------------------
def _r_own():
    """256 entries: exactly one k_mg_rank workgroup when the runs before it hold a multiple of 256."""
    return [(b"rank" + be64(1000 * j), V, _pat(j % 5, j), 10 ** 6 + j) for j in range(1, 257)]


def _r_other(window, salt, size=None):
    """A run with 3 entries below the own run's first key, `window` strictly between its first and last and
    the rest above (`size` entries in all, by default 3 more)."""
    cand = np.arange(1001, 256000)
    cand = cand[cand % 1000 != 0]
    mid = cand[np.linspace(salt, len(cand) - 1 - salt, window).astype(np.int64)]
    assert len(set(mid.tolist())) == window
    size = size or window + 6
    xs = [1, 2, 3] + mid.tolist() + [300000 + j for j in range(size - window - 3)]
    return [(b"rank" + be64(x), V, _pat(x % 4, x), 10 ** 5 * (salt + 1) + len(xs) - j) for j, x in enumerate(xs)]


def _r_windows(windows, own_last=False):
    def build():
        if own_last:  # the runs before the own one hold multiples of 256 entries
            others = [_r_other(c, 7 * j, (c + 3 + 255) // 256 * 256) for j, c in enumerate(windows)]
            return [make_run(r) for r in others + [_r_own()]], KEEP_ALL
        return [make_run(r) for r in [_r_own()] + [_r_other(c, 7 * j) for j, c in enumerate(windows)]], KEEP_ALL
    return build


def _r_ties():
    """Runs 0 and 1: the same 256 keys behind 12 shared bytes; run 2's outlier makes L0 0, so every window of
    runs 0 and 1 is equal.  A third of the keys carry the same seq in both runs."""
    a = [(b"tie-window--" + be32(j), V, _pat(j % 6, j), 900 + (j % 3 == 1)) for j in range(256)]
    b = [(b"tie-window--" + be32(j), V, _pat(j % 5, j + 1), 900 + (j % 3 == 2)) for j in range(256)]
    return [make_run(a), make_run(b), make_run([(b"\xff", V, b"outlier", 1)])], KEEP_ALL


R_SPARSE_SIZES = (0, 1, 0, 255, 0, 0, 257, 3, 1, 1, 1, 2, 0, 0, 5, 64, 0, 130, 7, 0, 256, 31, 0, 0, 12, 100, 1, 0, 9,
                  0, 40, 0)
assert len(R_SPARSE_SIZES) == _abi.MAX_RUNS


def _r_32(sizes, stride):
    def build():
        return [make_run([(b"sp" + be32(i * stride + r), V, _pat((i + r) % 6, i), 1000 + r) for i in range(n)])
                for r, n in enumerate(sizes)], KEEP_ALL
    return build


R_MIXED = {(1500, 1000, 500): (True, False, True), (1000, 1500, 500): (True, False, True),
           (500, 1000, 1500): (True, True, False)}


def r_cases():
    out = [Case("R/window-2048", ("window-lds-limit",), _r_windows((2048,)), window=2048, lds=True, twin="R/window-2049"),
           Case("R/window-2049", ("window-over-limit",), _r_windows((2049,)), window=2049, lds=False, twin="R/window-2048")]
    for w, lds in R_MIXED.items():
        out.append(Case("R/mixed-%d-%d-%d" % w, ("mixed-lds-hbm",), _r_windows(w), windows=w, lds=lds, own=0))
    out.append(Case("R/mixed-own-run-last", ("mixed-lds-hbm",), _r_windows((1500, 1000, 500), own_last=True),
                    windows=(1500, 1000, 500), lds=(True, False, True), own=3))
    out.append(Case("R/lds-ties", ("lds-ties-later-run", "lds-ties-earlier-run", "outlier"), _r_ties))
    out.append(Case("R/32-runs-sparse", ("workgroup-spans-runs", "empty-run"), _r_32(R_SPARSE_SIZES, 37)))
    out.append(Case("R/32-runs-dense", ("one-run-of-32",), _r_32((512,) * 32, 32)))
    return out


# ------------------------------------------------------------------------------------------------
# V: version walks
# ------------------------------------------------------------------------------------------------
V_HOT = b"hot"
V_TOP_SEQ = 100000


def v_seqs(nv):
    """Seqs of the hot key's versions, newest first: version j with j % 7 == 3 shares its seq with the next."""
    out, s = [], V_TOP_SEQ
    for j in range(nv):
        out.append(s)
        if j % 7 != 3:
            s -= 1
    return out


def _v_build(p, nv, nruns, tail, variant, tombs=0):
    def build():
        rows = [(j % nruns, (b"a%06d" % j, V, _pat(j % 4, j), 5)) for j in range(p)]
        for j, s in enumerate(v_seqs(nv)):
            if variant == "merge":
                row = (V_HOT, M, _pat(j % 40, j), s)
            elif j >= nv - tombs:
                row = (V_HOT, T, b"", s)
            elif variant == "expire" and j % 3 == 0:  # long values that expire: kept as tombstones
                row = (V_HOT, V, _pat(200 + j % 60, j), s, None, 10)
            else:
                row = (V_HOT, V, _pat(j % 40, j), s)
            rows.append((j % nruns, row))
        rows += [((p + j) % nruns, (b"z%06d" % j, V, _pat(j % 3, j), 5)) for j in range(tail)]
        ret = dict(KEEP_ALL)
        if variant == "none":
            ret = {}
        elif variant == "min-seq":
            ret = dict(min_seq=v_seqs(nv)[nv // 2])
        elif variant == "merge":
            ret = dict(merge_operands=True)
        elif variant == "expire":
            ret = dict(time_seq=0, compaction_start_ts=100)
        elif variant == "tomb-tail":
            ret = dict(time_seq=0, filter_tombstone=True)
        return [make_run(r) for r in _split(rows, nruns)], ret
    return build


# (p, nv, runs, single keys behind the hot key, variant[, tombstones at the old end])
V_SHAPES = (
    (0, 2, 2, 300, "keep"), (62, 3, 3, 300, "keep"), (63, 2, 2, 300, "keep"), (64, 65, 4, 300, "keep"),
    (254, 3, 2, 300, "keep"), (255, 257, 5, 300, "keep"), (256, 257, 3, 300, "keep"), (1022, 3, 3, 300, "keep"),
    (1023, 2, 2, 300, "keep"), (1023, 1025, 4, 300, "keep"), (1024, 2500, 5, 300, "keep"), (0, 2500, 3, 300, "keep"),
    (254, 65, 3, 0, "keep"), (1022, 1025, 2, 0, "keep"),
    (255, 257, 5, 300, "none"), (1023, 1025, 4, 300, "none"),
    (64, 65, 4, 300, "min-seq"), (1023, 1025, 4, 300, "min-seq"),
    (255, 257, 5, 300, "merge"), (1023, 2, 2, 300, "merge"), (1022, 1025, 2, 0, "merge"),
    (256, 257, 3, 300, "expire"), (1024, 2500, 5, 300, "expire"),
    (1022, 2500, 4, 300, "tomb-tail", 1500), (62, 3, 3, 300, "tomb-tail", 2),
)
V_PS = (0, 62, 63, 64, 254, 255, 256, 1022, 1023, 1024)
V_NVS = (2, 3, 65, 257, 1025, 2500)
V_VARIANT_CLAUSE = {"keep": "walk-keep-all", "none": "walk-newest-only", "min-seq": "walk-min-seq",
                    "merge": "walk-merge-operands", "expire": "walk-expiry-to-tombstone",
                    "tomb-tail": "walk-tombstone-tail"}
V_EDGES = (("wave", 64), ("workgroup", K_PFX_THREADS), ("tile", K_MERGE_TILE))


def v_edge_clauses(p, nv):
    """Which boundaries fall strictly inside positions [p, p + nv), and which sit at its start or its end."""
    out = []
    for name, step in V_EDGES:
        if any(x % step == 0 for x in range(p + 1, p + nv)):
            out.append("walk-%s-inside" % name)
        if p % step == 0 or (p + nv) % step == 0:
            out.append("walk-%s-at-end" % name)
    return out


def v_cases():
    out = []
    for shape in V_SHAPES:
        p, nv, nruns, tail, variant = shape[:5]
        tombs = shape[5] if len(shape) > 5 else 0
        clauses = [V_VARIANT_CLAUSE[variant]] + ["walk-equal-seqs"] * (nv >= 5) + v_edge_clauses(p, nv)
        if (p + nv - 1) // K_MERGE_TILE != p // K_MERGE_TILE and variant != "none":
            clauses.append("walk-other-tile-sums")  # kept versions past the tile of the walking thread's workgroup
        clauses += ["walk-first-overall"] * (p == 0) + ["walk-last-overall"] * (tail == 0)
        if variant == "tomb-tail" and (p + nv - tombs) // K_MERGE_TILE != (p + nv - 1) // K_MERGE_TILE:
            clauses.append("tombstone-tail-crosses-tile")
        out.append(Case("V/p%d-nv%d-%s%s" % (p, nv, variant, "-last" if not tail else ""), clauses,
                        _v_build(p, nv, nruns, tail, variant, tombs), p=p, nv=nv, variant=variant, tombs=tombs))
    return out


# ------------------------------------------------------------------------------------------------
# S: tiles
# ------------------------------------------------------------------------------------------------
S_TOTALS = (1, 1023, 1024, 1025)
S_BIG_KEYS = 450000        # counters; every fifth also has an older version in the other run
S_BIG_TOTAL = S_BIG_KEYS + S_BIG_KEYS // 5
assert S_BIG_TOTAL >= K_MERGE_THREADS * K_MERGE_TILE + 1


def _s_small(total):
    def build():
        rows = [(j % 2, (b"s%07d" % j, V, _pat(j % 3, j), 100 + j)) for j in range(total)]
        return [make_run(r) for r in _split(rows, 2)], KEEP_ALL
    return build


def _s_big():
    """Two runs of interleaved 8-byte big-endian counters behind 12 shared bytes, values of 0 to 2 bytes; counter
    x lives in run x % 2 and, when x % 5 == 0, an older version in the other run, which retention drops; every
    ninth newest version is a tombstone, dropped by filter_tombstone when it is the key's only kept version."""
    x = np.arange(S_BIG_KEYS, dtype=np.uint64)
    dup = x[x % 5 == 0]
    runs = []
    for r in (0, 1):
        new, old = x[x % 2 == r], dup[dup % 2 != r]
        c = np.concatenate([new, old])
        seq = np.concatenate([new + np.uint64(10 ** 6), old + np.uint64(10)])
        o = np.argsort(c, kind="stable")  # a counter is in a run once: new or old
        c, seq = c[o], seq[o]
        n = len(c)
        kb = np.empty((n, 20), np.uint8)
        kb[:, :12] = np.frombuffer(b"scan-carry--", np.uint8)
        kb[:, 12:] = c.byteswap().view(np.uint8).reshape(-1, 8)
        tomb = (c % 9 == 4) & (seq >= 10 ** 6)
        vlen = np.where(tomb, 0, c % 3).astype(np.uint32)
        voff = np.concatenate([[0], np.cumsum(vlen)[:-1]]).astype(np.uint64)
        vb = ((np.arange(int(vlen.sum()) + 1) * 7 + r) % 253).astype(np.uint8)
        runs.append(Run(kb.reshape(-1), np.arange(n + 1, dtype=np.uint64) * np.uint64(20), vb, voff, vlen, seq,
                        np.where(tomb, _abi.FLAG_TOMBSTONE, 0).astype(np.uint8), np.zeros(n, np.int64),
                        np.zeros(n, np.int64)))
    return runs, dict(filter_tombstone=True)


def s_cases():
    out = [Case("S/total-%d" % t, ("tile-count",), _s_small(t), tiles=(t + 1023) // 1024) for t in S_TOTALS]
    out.append(Case("S/scan-carry", ("scan-second-pass", "lcp0"), _s_big, big=True,
                    tiles=(S_BIG_TOTAL + 1023) // 1024, L0=12 + 5))  # counters below 2^24: five zero bytes more
    return out


def s_capacity_case():
    """The case whose outputs are one short of each capacity in turn (tests/test_gpu_merge_edges.py)."""
    return Case("S/capacity", ("capacity",), _s_small(1025), tiles=2)


# ------------------------------------------------------------------------------------------------
# C: byte copies
# ------------------------------------------------------------------------------------------------
C_LENS = (0, 1, 7, 8, 15, 16, 17, 31, 32, 33, 127, 128, 129, 143, 144, 145, 255, 256, 257, 300, 4097)
C_SHORT = (7, 8, 15, 16, 17, 31, 32, 33)
C_ROUNDS = 3
C_GROUPS = ("mk<mv", "mk>mv", "mk==mv", "long-among-short", "long-value-among-short", "mixed")


def c_lengths(limit=4097, head=True):
    """(key length, value length, tombstone carrying bytes?) per merged position: C_ROUNDS rounds of six copy
    groups of 64.  Key lengths 0 and 1 stand at the stream's start (`head`; position i's key is otherwise a 2-byte
    big-endian 0x0100 + i, padded to its length)."""
    lens = [x for x in C_LENS if x <= limit]
    long_k = [x for x in lens if x >= 7]
    top = max(lens)
    mid = max(x for x in lens if x <= 300)
    mid_k, mid_v = [x for x in long_k if x <= mid], [x for x in lens if x <= mid]
    out = []
    for rnd in range(C_ROUNDS):
        for j in range(64):  # short keys, every value length
            out.append((C_SHORT[(j + rnd) % 8], lens[(j + 5 * rnd) % len(lens)]))
        for j in range(64):  # every key length, short values
            out.append((long_k[(j + 3 * rnd) % len(long_k)], j % 2 if j % 5 == 0 else C_SHORT[(j + rnd) % 8]))
        for j in range(64):  # both up to the same maximum
            out.append((mid_k[(j + rnd) % len(mid_k)], mid_v[(j * 7 + rnd) % len(mid_v)]))
        for j in range(64):  # one long entry among short ones
            out.append((top, top) if j == 21 + rnd else (8, 7))
        for j in range(64):  # one long value among short ones
            out.append((16, mid) if j == 63 - rnd else (16, 1))
        for j in range(64):  # strides coprime with both lists' lengths
            out.append((long_k[(j * 5 + rnd) % len(long_k)], lens[(j * 11 + rnd) % len(lens)]))
    if head:
        out[0], out[1] = (0, mid), (1, 33)
    # tombstones whose val_len is not 0: every 13th position (their bytes are ignored, the copy sees no value)
    return [(kl, vl, i % 13 == 6 and vl > 0) for i, (kl, vl) in enumerate(out)]


def _c_build(limit=4097, v0s=(0, 5), head=True):
    def build():
        rows = []
        for i, (kl, vl, tomb) in enumerate(c_lengths(limit, head)):
            key = (struct.pack(">H", 0x0100 + i) + _pat(max(kl - 2, 0), i))[:kl] if kl >= 2 else (b"", b"\x00")[kl]
            rows.append(((i // 3) % 2, (key, T if tomb else V, _pat(vl, i + 1), 50 + i, None, None)))
        return [make_run(r, k0=k0, v0=v0) for r, k0, v0 in zip(_split(rows, 2), (0, 3), v0s)], KEEP_ALL
    return build


C_CLAUSES = ("copy-lengths", "copy-mk<mv", "copy-mk>mv", "copy-mk==mv", "copy-long-among-short", "copy-steps",
             "value-source-residues", "tombstone-carries-bytes")


def c_cases():
    cl = C_CLAUSES + ("empty-first-key",)
    return [Case("C/lengths", cl, _c_build(), limit=4097, head=True),
            Case("C/lengths-other-residues", cl, _c_build(v0s=(9, 14)), limit=4097, head=True)]


def c_sst_case():
    """Family C inside the SST format's limits (for the end-to-end compactor runs): lengths up to 300, no empty key."""
    return Case("C/lengths-to-300", C_CLAUSES, _c_build(300, head=False), limit=300, head=False)


# ------------------------------------------------------------------------------------------------
CLAUSES = (
    # K
    "lcp0", "short-keys", "window-ties", "prefix-keys", "zero-tails", "high-bytes", "empty-first-key", "outlier",
    "empty-run", "load8-residues", "order-after-8", "order-seq", "order-two",
    # R
    "window-lds-limit", "window-over-limit", "mixed-lds-hbm", "lds-ties-later-run", "lds-ties-earlier-run",
    "workgroup-spans-runs", "one-run-of-32",
    # V
    "walk-keep-all", "walk-newest-only", "walk-min-seq", "walk-merge-operands", "walk-expiry-to-tombstone",
    "walk-tombstone-tail", "tombstone-tail-crosses-tile", "walk-equal-seqs", "walk-other-tile-sums", "walk-first-overall",
    "walk-last-overall",
    "walk-wave-inside", "walk-wave-at-end", "walk-workgroup-inside", "walk-workgroup-at-end", "walk-tile-inside",
    "walk-tile-at-end",
    # S
    "tile-count", "scan-second-pass", "capacity",
    # C
    "copy-lengths", "copy-mk<mv", "copy-mk>mv", "copy-mk==mv", "copy-long-among-short", "copy-steps",
    "value-source-residues", "tombstone-carries-bytes",
)


def all_cases():
    """Every case one sdb_merge_runs call takes."""
    return k_cases() + r_cases() + v_cases() + s_cases() + [s_capacity_case()] + c_cases() + [c_sst_case()]


def compactor_only_cases():
    """More than SDB_MAX_RUNS runs: a compactor job only."""
    return [k_many_runs()]


def clause_table(cases=None):
    table = {c: [] for c in CLAUSES}
    for case in cases or all_cases() + compactor_only_cases():
        for c in case.clauses:
            table[c].append(case.name)
    return table
