"""The hand-shaped merge cases (tests/merge_cases.py) reach what they claim, on the CPU: the restatement of the
device's decisions (L0, windows, rank windows and their LDS placement, version walks, tiles, copy groups) shows
every case on the clause it names and its neighbour on the other side, every clause has a case, and the oracle
(the judge of tests/test_gpu_merge_edges.py) agrees with py_merge / py_retention on exactly these shapes."""
import numpy as np
import pytest

from slatedb_amd import _abi

from . import merge_cases as Mc
from .test_compaction_oracle import entries_of, py_merge, py_retention

CASES = Mc.all_cases() + Mc.compactor_only_cases()
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]


def _all_keys(st):
    return sorted({k for ks in st.keys for k in ks})


def _violations(case):
    """Every global entry that breaks its run's order (key asc, seq desc)."""
    out, base = [], 0
    for r in case.runs:
        ks, sq = Mc.keys_of(r), r.seq.tolist()
        out += [base + i for i in range(1, r.n) if ks[i - 1] > ks[i] or (ks[i - 1] == ks[i] and sq[i - 1] < sq[i])]
        base += r.n
    return out


def _entry(case, g):
    for r in case.runs:
        if g < r.n:
            return Mc.keys_of(r)[g], int(r.seq[g])
        g -= r.n


def _hot(st):
    assert len(st.walks) == 1, len(st.walks)
    return st.walks[0]


# ------------------------------------------------------------------------------------------------
# one check per clause: (case, its restated state) -> asserts
# ------------------------------------------------------------------------------------------------
def _lcp0(c, st):
    assert st.L0 == c.expect["L0"], st.L0


def _short_keys(c, st):
    lens = {len(k) - st.L0 for k in _all_keys(st)}
    assert set(range(0, 10)) <= lens and max(lens) >= 40, sorted(lens)  # 0, 1 .. 7, 8, 9 and longer


def _window_ties(c, st):
    ks = _all_keys(st)
    first_diff = {Mc.lcp(a, b) - st.L0 for a, b in zip(ks, ks[1:])
                  if Mc.window(a, st.L0) == Mc.window(b, st.L0) and Mc.lcp(a, b) < min(len(a), len(b))}
    assert first_diff and min(first_diff) >= 8, sorted(first_diff)  # tied windows, decided by later bytes
    if "L0" in c.name:
        assert set(Mc.K_DIFF_AT) <= first_diff, sorted(first_diff)


def _prefix_keys(c, st):
    ks = _all_keys(st)
    ends = {len(a) - st.L0 for a, b in zip(ks, ks[1:]) if len(a) < len(b) and b.startswith(a)}
    assert {2, 8, 9} <= ends and any(e > 9 for e in ends) and any(e < 8 for e in ends), sorted(ends)


def _zero_tails(c, st):
    ks = set(_all_keys(st))
    pre = Mc.k_prefix(st.L0)
    for stem in Mc.K_ZERO_STEMS:
        assert all(pre + stem + b"\0" * j in ks for j in range(10)), stem
    # in the zero-padded window k and k + \0 are equal: their order comes from the lengths
    tied = [(a, b) for a, b in zip(sorted(ks), sorted(ks)[1:])
            if b == a + b"\0" and len(b) <= st.L0 + 8 and Mc.window(a, st.L0) == Mc.window(b, st.L0)]
    assert len(tied) >= 8


def _high_bytes(c, st):
    assert {0x7F, 0x80, 0xFF} <= {k[st.L0] for k in _all_keys(st) if len(k) > st.L0}


def _empty_first_key(c, st):
    assert st.keys[0][0] == b""


def _outlier(c, st):
    """L0 is 0 although every key but one shares at least 12 bytes: all windows but the outlier's tie."""
    ks = _all_keys(st)
    assert st.L0 == 0 and Mc.lcp(ks[0], ks[-2]) >= 12 and Mc.lcp(ks[0], ks[-1]) == 0
    assert len(set(st.win.tolist())) == 2 and int((st.win == st.win[0]).sum()) == st.total - 1


def _empty_run(c, st):
    sizes = [r.n for r in c.runs]
    assert 0 in sizes and any(sizes)
    if "sparse" in c.name:  # first, last and consecutive
        assert sizes[0] == 0 and sizes[-1] == 0 and any(a == b == 0 for a, b in zip(sizes[1:-1], sizes[2:-1]))


def _load8_residues(c, st):
    every = set(range(8))
    starts = [int(o) for r in c.runs for o in r.key_off[:-1]]
    assert {r.key_off[0] for r in c.runs} == set(Mc.K_RES_K0)
    assert {o % 8 for o in starts} == every                      # key_prefix of the whole key (the order check)
    assert {(o + st.L0) % 8 for o in starts} == every            # the window
    assert {(o + st.L0 + 8) % 8 for o in starts} == every        # cmp_key's bytes after a tied window
    assert len(set(st.win.tolist())) == 3


def _order_after_8(c, st):
    (g,) = _violations(c)
    assert g == st.error == c.expect["entry"]
    (a, _), (b, _) = _entry(c, g - 1), _entry(c, g)
    assert a > b and Mc.lcp(a, b) >= c.expect["equal"] >= 8 and a[:8] == b[:8]


def _order_seq(c, st):
    (g,) = _violations(c)
    assert g == st.error == c.expect["entry"]
    (a, sa), (b, sb) = _entry(c, g - 1), _entry(c, g)
    assert a == b and len(a) > 16 and sa < sb
    assert sum(k == a for k in c.state.keys[1]) >= 300


def _order_two(c, st):
    v = _violations(c)
    assert tuple(v) == c.expect["all_errors"] and st.error == min(v) == c.expect["entry"]
    assert v[0] // Mc.K_PFX_THREADS != v[1] // Mc.K_PFX_THREADS
    for g in v:
        (a, _), (b, _) = _entry(c, g - 1), _entry(c, g)
        assert a[:8] == b[:8]


def _window_limit(c, st):
    g = st.groups[0]
    assert g["one_run"] and g["run"] == 0 and c.runs[0].n == Mc.K_PFX_THREADS
    assert g["win"] == {1: c.expect["window"]} and g["lds"] == {1: c.expect["lds"]}
    assert c.expect["lds"] == (c.expect["window"] <= Mc.K_RANK_LDS_PREFIXES)
    t = BY_NAME[c.expect["twin"]]
    tg = t.state.groups[0]
    assert abs(tg["win"][1] - g["win"][1]) == 1 and tg["lds"][1] != g["lds"][1]


def _mixed(c, st):
    own = c.expect["own"]
    assert st.bases[own] % Mc.K_PFX_THREADS == 0 and c.runs[own].n == Mc.K_PFX_THREADS
    g = st.groups[st.bases[own] // Mc.K_PFX_THREADS]
    others = [r for r in range(st.nruns) if r != own]
    assert g["one_run"] and g["run"] == own
    assert tuple(g["win"][r] for r in others) == c.expect["windows"]
    assert tuple(g["lds"][r] for r in others) == c.expect["lds"]
    # a window that does not fit is left out and a later, smaller one is still packed; or the last one overflows
    assert set(c.expect["lds"]) == {True, False}


def _lds_ties(own, other):
    def check(c, st):
        g = st.groups[own]
        assert g["one_run"] and g["run"] == own and g["lds"][other] and g["win"][other] >= 200
        a, b = st.bases[own], st.bases[other]
        assert len(set(st.win[a:a + 256].tolist()) | set(st.win[b:b + 256].tolist())) == 1  # every LDS step ties
        mine = set(zip(st.keys[own], c.runs[own].seq.tolist()))
        same = mine & set(zip(st.keys[other], c.runs[other].seq.tolist()))
        assert len(same) >= 50  # equal (key, seq) pairs: the run order decides
    return check


def _spans(c, st):
    assert st.nruns == _abi.MAX_RUNS
    assert any(not g["one_run"] and g["spans"] >= 5 for g in st.groups)
    assert any(g["one_run"] for g in st.groups)


def _one_run_32(c, st):
    assert st.nruns == _abi.MAX_RUNS and all(g["one_run"] for g in st.groups)
    assert all(len(g["win"]) == 31 for g in st.groups)
    assert all({True, False} == set(g["lds"].values()) for g in st.groups)


def _walk_shape(c, st):
    w = _hot(st)
    assert (w["p"], w["nv"]) == (c.expect["p"], c.expect["nv"])
    assert c.expect["p"] in Mc.V_PS and c.expect["nv"] in Mc.V_NVS
    edges = {x for x in c.clauses if x.endswith("-inside") or x.endswith("-at-end")}
    assert edges == set(Mc.v_edge_clauses(w["p"], w["nv"]))
    return w


def _walk_edge(name, step, inside):
    def check(c, st):
        w = _walk_shape(c, st)
        p, e = w["p"], w["p"] + w["nv"]
        if inside:  # positions m - 1 and m both belong to the walk
            assert any(p < m < e for m in range(0, e + step, step))
        else:
            assert p % step == 0 or e % step == 0
    return check


def _kept(w):
    return sum(d != 0 for d in w["dec"])


def _walk_keep_all(c, st):
    w = _walk_shape(c, st)
    assert _kept(w) == w["nv"] - w["equal_seqs"] and (c.expect["tombs"] == 0)


def _walk_newest_only(c, st):
    w = _walk_shape(c, st)
    assert _kept(w) == 1


def _walk_min_seq(c, st):
    w = _walk_shape(c, st)
    k = max(i for i, d in enumerate(w["dec"]) if d)
    assert w["nv"] // 4 < k < w["nv"] - 2 and not any(w["dec"][k + 1:])  # the walk continues, then breaks


def _walk_merge(c, st):
    w = _walk_shape(c, st)
    flags = [int(c.runs[r].flags[i]) for r, i in st.order[w["p"]:w["p"] + w["nv"]]]
    assert all(f & _abi.FLAG_MERGE_OPERAND for f in flags) and c.ret.merge_operands
    assert _kept(w) == w["nv"] - w["equal_seqs"]


def _walk_expiry(c, st):
    w = _walk_shape(c, st)
    conv = [q for q in range(w["p"], w["p"] + w["nv"]) if st.dec[q] == 2]
    assert len(conv) >= w["nv"] // 5 and st.expired_values >= len(conv)
    assert all(int(c.runs[r].val_len[i]) >= 200 for r, i in (st.order[q] for q in conv))
    assert all(st.vb[q] == 0 for q in conv)


def _walk_tomb_tail(c, st):
    w = _walk_shape(c, st)
    t = c.expect["tombs"]
    assert t and not any(w["dec"][-t:]) and w["dec"][-t - 1]
    assert _kept(w) == w["nv"] - t - sum(1 for i in range(w["nv"] - t - 1) if Mc.v_seqs(w["nv"])[i] == Mc.v_seqs(w["nv"])[i + 1])


def _tomb_tail_tile(c, st):
    w = _walk_shape(c, st)
    e, t = w["p"] + w["nv"], c.expect["tombs"]
    assert (e - t) // Mc.K_MERGE_TILE != (e - 1) // Mc.K_MERGE_TILE


def _walk_equal_seqs(c, st):
    assert _hot(st)["equal_seqs"] >= 1


def _walk_other_tile(c, st):
    w = _hot(st)
    assert set(w["tiles"]) - {w["p"] // Mc.K_MERGE_TILE}


def _walk_first(c, st):
    assert _hot(st)["p"] == 0


def _walk_last(c, st):
    w = _hot(st)
    assert w["p"] + w["nv"] == st.total


def _tile_count(c, st):
    assert st.ntiles == c.expect["tiles"]


def _scan_second_pass(c, st):
    assert st.ntiles == c.expect["tiles"] > Mc.K_MERGE_THREADS and st.total >= Mc.K_MERGE_THREADS * Mc.K_MERGE_TILE + 1
    _, sm = c.ref
    assert sm.status == 0 and 0 < sm.num_out < sm.num_in  # retention drops some


def _capacity(c, st):
    _, sm = c.ref
    assert sm.status == 0 and sm.num_out > Mc.K_MERGE_TILE and sm.key_bytes and sm.val_bytes


def _copy_lengths(c, st):
    lens = {x for x in Mc.C_LENS if x <= c.expect["limit"]}
    assert all(st.dec)
    assert lens - (set() if c.expect["head"] else {0, 1}) <= set(st.kb)
    assert lens <= set(st.vb)
    assert st.kb == [kl for kl, _, _ in Mc.c_lengths(c.expect["limit"], c.expect["head"])]  # position i is entry i


def _copy_group(pred):
    def check(c, st):
        hits = [g for g in st.copy if pred(g, st)]
        assert len(hits) >= Mc.C_ROUNDS, len(hits)
        assert {g["start"] // (Mc.K_MERGE_TILE // 2) for g in hits} >= {0, 1}  # in both halves of a tile
    return check


def _long_among_short(g, st):
    kb, vb = st.kb[g["start"]:g["start"] + 64], st.vb[g["start"]:g["start"] + 64]
    return g["mk"] >= 300 and sorted(kb)[-2] <= 16 and g["mv"] >= 300 and sorted(vb)[-2] <= 16


def _copy_steps(c, st):
    assert any(g["joint"] >= 2 for g in st.copy)                          # the 128-byte step taken again
    assert any(g["joint"] and g["key_steps"] and not g["val_steps"] for g in st.copy)   # a separate key tail
    assert any(g["joint"] and g["val_steps"] and not g["key_steps"] for g in st.copy)   # a separate value tail
    assert any(g["mk"] > 4096 for g in st.copy) == (c.expect["limit"] > 4096)


def _value_residues(c, st):
    res16 = {int(o) % 16 for r in c.runs for o, n, f in zip(r.val_off, r.val_len, r.flags)
             if n >= 16 and not f & _abi.FLAG_TOMBSTONE}
    short = {int(o) % 16 for r in c.runs for o, n, f in zip(r.val_off, r.val_len, r.flags)
             if 0 < n < 16 and not f & _abi.FLAG_TOMBSTONE}
    assert res16 == set(range(16)) and len(short) >= 8, (sorted(res16), sorted(short))


def _tomb_carries(c, st):
    n = sum(int(((r.flags & _abi.FLAG_TOMBSTONE) != 0).astype(int) @ (r.val_len > 0).astype(int)) for r in c.runs)
    assert n >= 20
    tomb_pos = [q for q, (r, i) in enumerate(st.order) if int(c.runs[r].flags[i]) & _abi.FLAG_TOMBSTONE]
    assert all(st.vb[q] == 0 for q in tomb_pos)


CHECKS = {
    "lcp0": _lcp0, "short-keys": _short_keys, "window-ties": _window_ties, "prefix-keys": _prefix_keys,
    "zero-tails": _zero_tails, "high-bytes": _high_bytes, "empty-first-key": _empty_first_key, "outlier": _outlier,
    "empty-run": _empty_run, "load8-residues": _load8_residues, "order-after-8": _order_after_8,
    "order-seq": _order_seq, "order-two": _order_two,
    "window-lds-limit": _window_limit, "window-over-limit": _window_limit, "mixed-lds-hbm": _mixed,
    "lds-ties-later-run": _lds_ties(0, 1), "lds-ties-earlier-run": _lds_ties(1, 0),
    "workgroup-spans-runs": _spans, "one-run-of-32": _one_run_32,
    "walk-keep-all": _walk_keep_all, "walk-newest-only": _walk_newest_only, "walk-min-seq": _walk_min_seq,
    "walk-merge-operands": _walk_merge, "walk-expiry-to-tombstone": _walk_expiry,
    "walk-tombstone-tail": _walk_tomb_tail, "tombstone-tail-crosses-tile": _tomb_tail_tile,
    "walk-equal-seqs": _walk_equal_seqs, "walk-other-tile-sums": _walk_other_tile,
    "walk-first-overall": _walk_first, "walk-last-overall": _walk_last,
    "walk-wave-inside": _walk_edge("wave", 64, True), "walk-wave-at-end": _walk_edge("wave", 64, False),
    "walk-workgroup-inside": _walk_edge("workgroup", 256, True),
    "walk-workgroup-at-end": _walk_edge("workgroup", 256, False),
    "walk-tile-inside": _walk_edge("tile", 1024, True), "walk-tile-at-end": _walk_edge("tile", 1024, False),
    "tile-count": _tile_count, "scan-second-pass": _scan_second_pass, "capacity": _capacity,
    "copy-lengths": _copy_lengths,
    "copy-mk<mv": _copy_group(lambda g, st: 0 < g["mk"] < g["mv"]),
    "copy-mk>mv": _copy_group(lambda g, st: g["mk"] > g["mv"] > 0),
    "copy-mk==mv": _copy_group(lambda g, st: g["mk"] == g["mv"] > 128),
    "copy-long-among-short": _copy_group(_long_among_short), "copy-steps": _copy_steps,
    "value-source-residues": _value_residues, "tombstone-carries-bytes": _tomb_carries,
}


def test_constants_are_the_sources():
    """The constants the restatement uses, as sdb_compact.hip / sdb_compact.h spell them."""
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "slatedb_amd", "csrc")
    src = open(os.path.join(root, "sdb_compact.hip")).read() + open(os.path.join(root, "sdb_compact.h")).read()
    assert re.search(r"constexpr uint32_t kPfxThreads = %d;" % Mc.K_PFX_THREADS, src)
    assert re.search(r"constexpr uint32_t kRankLds = %d \* 1024;" % (Mc.K_RANK_LDS_PREFIXES * 8 // 1024), src)
    assert re.search(r"#define SDB_MERGE_TILE %d\b" % Mc.K_MERGE_TILE, src)
    assert re.search(r"#define SDB_MERGE_THREADS %d\b" % Mc.K_MERGE_THREADS, src)
    assert "x0 += %d" % Mc.K_COPY_STEP in src and "%d * (l & 7)" % Mc.K_CHUNK in src


def test_every_clause_has_a_case():
    table = Mc.clause_table(CASES)
    assert set(table) == set(Mc.CLAUSES) == set(CHECKS)
    empty = [c for c, names in table.items() if not names]
    assert not empty, empty
    assert len(BY_NAME) == len(CASES)
    fam = {f: sum(c.name.startswith(f + "/") for c in CASES) for f in "KRVSC"}
    assert fam == dict(K=25, R=9, V=25, S=6, C=3), fam


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_sits_on_its_clauses(case):
    st = case.state
    assert case.clauses
    for clause in case.clauses:
        CHECKS[clause](case, st)
    _, sm = case.ref
    if "status" in case.expect:  # an order error: the oracle reports the restated entry
        assert (sm.status, sm.first_error_entry) == (case.expect["status"], case.expect["entry"]) and st.error == case.expect["entry"]
    else:
        assert sm.status == 0 and st.error is None and sm.num_in == st.total


def test_neighbours_sit_on_the_other_side():
    a, b = BY_NAME["R/window-2048"].state.groups[0], BY_NAME["R/window-2049"].state.groups[0]
    assert (a["win"][1], a["lds"][1], b["win"][1], b["lds"][1]) == (2048, True, 2049, False)
    # p = 255 starts the walk on the last thread of workgroup 0, p = 256 on the first of workgroup 1; 63 / 64 and
    # 1023 / 1024 likewise for waves and tiles
    for lo, hi, step in (("V/p255-nv257-keep", "V/p256-nv257-keep", 256), ("V/p63-nv2-keep", "V/p64-nv65-keep", 64),
                         ("V/p1023-nv1025-keep", "V/p1024-nv2500-keep", 1024)):
        pl, ph = _hot(BY_NAME[lo].state)["p"], _hot(BY_NAME[hi].state)["p"]
        assert pl + 1 == ph and pl % step == step - 1 and ph % step == 0
    tiles = {c.expect["tiles"] for c in CASES if c.name.startswith("S/total")}
    assert tiles == {1, 2} and BY_NAME["S/total-1024"].state.ntiles + 1 == BY_NAME["S/total-1025"].state.ntiles
    # the mixed placements differ between the orders
    assert len({(c.expect["windows"], c.expect["lds"]) for c in CASES if c.name.startswith("R/mixed")}) == 3


def test_v_pairs_cover_every_edge_both_ways():
    ps, nvs = {c.expect["p"] for c in Mc.v_cases()}, {c.expect["nv"] for c in Mc.v_cases()}
    assert ps == set(Mc.V_PS) and nvs == set(Mc.V_NVS)
    runs = {len(c.runs) for c in Mc.v_cases()}
    assert runs == {2, 3, 4, 5}


@pytest.mark.parametrize("case", [c for c in CASES if not c.big], ids=[c.name for c in CASES if not c.big])
def test_oracle_equals_python_restatement(case):
    """The oracle's merged stream and summary against py_merge / py_retention (and the restated decisions)."""
    merged, sm = case.ref
    st, ret = case.state, case.ret
    if st.error is not None:
        assert sm.status == _abi.SDB_INVALID_ARGUMENT and sm.first_error_entry == st.error
        return
    want = py_retention(py_merge([Mc.entries_of_run(r) for r in case.runs]), ret.min_seq if ret.has_min_seq else None,
                        ret.time_seq if ret.has_time_window else None, ret.compaction_start_ts, bool(ret.filter_tombstone))
    assert entries_of(merged) == want
    assert (sm.status, sm.num_in, sm.num_out) == (0, st.total, len(want))
    assert sm.key_bytes == sum(len(e[0]) for e in want) == sum(st.kb)
    assert sm.val_bytes == sum(len(e[2]) for e in want) == sum(st.vb)
    assert (sm.expired_values, sm.expired_merges) == (st.expired_values, st.expired_merges)
    assert sm.num_out == sum(d != 0 for d in st.dec)
    assert np.array_equal(merged.key_off, np.concatenate([[0], np.cumsum([k for k, d in zip(st.kb, st.dec) if d])]))


def test_scan_carry_case_by_construction():
    """The 540 000-entry case is too large for py_merge: its output is known from how it is built."""
    c = BY_NAME["S/scan-carry"]
    merged, sm = c.ref
    x = np.arange(Mc.S_BIG_KEYS, dtype=np.uint64)
    live = x[x % 9 != 4]  # the newest version of every counter, unless it is a tombstone (filtered)
    assert sm.status == 0 and sm.num_in == Mc.S_BIG_TOTAL and sm.num_out == len(live)
    assert np.array_equal(merged.key_bytes.reshape(-1, 20)[:, 12:].copy().view(">u8").reshape(-1), live)
    assert np.array_equal(merged.seq, live + np.uint64(10 ** 6))
    assert np.array_equal(np.diff(merged.val_off), live % 3) and sm.val_bytes == int((live % 3).sum())
