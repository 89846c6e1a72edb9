"""The hand-shaped encoder cases (tests/encode_cases.py) reach what they claim, on the CPU oracle: the
clause each routing case names has the stated value and decides the route, the twin one step away takes
another route, the k_facts lattice lands on the lanes it is meant for, and a tombstone's ignored bytes
change nothing in the encoded SST."""
import numpy as np

from oracle import oracle as O

from . import encode_cases as E

IMAGE_CLAUSES = ("ne", "bb", "nv16", "nk16")


def _failing(r):
    """The clauses of emit_fast that a block fails."""
    lim = dict(ne=64, bb=E.IMG_CAP - 64, nv16=E.STAGE_CAP // 16, nk16=E.KEY_STAGE_CAP // 16)
    return [c for c in IMAGE_CLAUSES if r[c] > lim[c]]


def _same_sst(a, b, what):
    assert a.status == b.status == 0, what
    for f, _ in type(a.summary)._fields_:
        assert getattr(a.summary, f) == getattr(b.summary, f), (what, f)
    for f in ("data", "block_off", "block_first_entry", "index_key_len", "block_stats", "bloom"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


def test_r_cases_sit_on_their_clause():
    cases = E.r_cases()
    assert len(cases) == 25 * len(E.FORMATS)
    by_name = {c.name: c for c in cases}
    assert len(by_name) == len(cases)
    seen = set()
    for c in cases:
        ref = c.ref()
        assert ref.status == 0, c.name
        routes = c.routes(ref)
        x = c.expect
        r = routes[E.target_block(c, routes)]
        assert r["route"] == x["route"], (c.name, r)
        seen.add(r["route"])
        assert not r["carry"], c.name
        clause, fails = x["clause"], _failing(r)
        if clause in IMAGE_CLAUSES:
            assert r[clause] == x["value"], (c.name, r)
            assert fails == ([] if x["route"] == "image" else [clause]), (c.name, fails)  # that clause alone decides
        else:
            assert fails and x["route"] != "image", (c.name, r)  # the piece limits matter off the image path only
            assert r["huge"] == (x["route"] == "workgroup"), (c.name, r)
            if clause != "huge":  # exactly one row at the stated size, and no other fact over its limit
                f = E.facts(c.batch, c.version)
                assert f[clause][x["row"]] == x["value"], (c.name, f[clause][x["row"]])
                over = (f["s_r"] > E.PIECE_ROW_MAX) | (f["klen"] > E.PIECE_KEY_MAX) | (f["vlen"] > E.PIECE_VAL_MAX)
                assert over.sum() == (x["route"] == "workgroup") and not np.delete(over, x["row"]).any(), c.name
        if "all_routes" in x:
            off_image = [q["route"] for q in routes if _failing(q)]  # (a short last block may fit the image)
            assert set(off_image) == {x["all_routes"]} and len(off_image) >= 2, c.name
        if x["twin"] is not None:  # one step away the route flips
            t = by_name[x["twin"]]
            tr = t.routes()
            q = tr[E.target_block(t, tr)]
            assert q["route"] != r["route"], (c.name, t.name)
            if clause in IMAGE_CLAUSES:
                assert abs(q[clause] - r[clause]) == 1, (c.name, q[clause], r[clause])
            elif clause != "huge":
                assert abs(t.expect["value"] - x["value"]) == 1, c.name
    assert seen == {"image", "pieces", "workgroup"}


def test_r_framing_and_chunk_edges():
    """The framed target is block 1 of 3; the chunk cases have a block ending at, and one straddling, entry 2048."""
    for c in E.r_cases():
        routes = c.routes()
        if c.expect["block"] == 1:
            assert len(routes) == 3 and routes[0]["ne"] == routes[2]["ne"] == 1, c.name
        elif c.expect["block"] == "ends-at-2048":
            k = E.target_block(c, routes)
            assert routes[k]["ne"] > 64 and routes[k + 1]["s"] == E.CHUNK and routes[k + 1]["route"] == "workgroup", c.name
            assert all(q["route"] == "pieces" for q in routes[:k + 1]), c.name
        elif c.expect["block"] == "straddles-2048":
            k = E.target_block(c, routes)
            assert all(q["route"] == "pieces" for q in routes[:k]) and k >= 1, c.name
            assert all(q["route"] == "workgroup" for q in routes[k:]), c.name


def test_t_cases_equal_their_stripped_twins():
    cases = E.t_cases()
    per_off = len(E.T_PAYLOADS) * len(E.T_POSITIONS)
    assert len(cases) == 2 * 2 * 2 * (len(E.T_OFFSETS) * per_off + len(E.T_OFFSETS) - 1 + 2 * len(E.T_SPAN_VLENS))
    seen = set()
    for c in cases:
        ref = c.ref()
        twin = E.stripped(c.batch)
        assert not twin.key_off[0] and not twin.val_off[0]
        _same_sst(ref, O.encode_sst(twin, O.params(**c.kw)), c.name)
        routes = c.routes(ref)
        seen |= {r["route"] for r in routes}
        f = E.facts(c.batch, c.version)
        carriers = np.nonzero(f["tomb"] & (f["vraw"] > 0))[0]
        x = c.expect
        if x["position"] is None:
            assert carriers.size == 0 and int(c.batch.key_off[0]) in E.T_OFFSETS[1:], c.name
            assert not any(r["carry"] for r in routes), c.name
            continue
        assert carriers.size == 1 and f["vraw"][carriers[0]] == x["payload"], c.name
        s, e = routes[1]["s"], routes[1]["e"]
        at = int(carriers[0])
        assert {"first": at == s, "middle": s < at < e - 1, "last": at == e - 1}[x["position"]], (c.name, at, s, e)
        assert all(r["route"] == "workgroup" for r in routes), c.name  # one chunk: every block follows the flag
        if "spans" in c.name:  # behind the carrier, values too long for k_emit's register copy, staged above their rows
            b = c.batch
            staged = lambda r: int(b.val_off[r]) - (int(b.val_off[s]) & ~15) - 64  # offset from the image's first byte
            image_max = lambda r: int(f["s_r"][s:r].sum()) + 40                    # rows before it, its header and key
            above = [r for r in range(at + 1, e) if f["vlen"][r] > 108 and staged(r) > image_max(r)]
            assert len(above) >= 2, c.name
    assert seen == {"image", "pieces", "workgroup"}


def test_t_payload_over_a_stage_is_what_the_piece_path_cannot_take():
    """The 4097-byte payload at 16 KiB is the case the piece path has no room for: the row's raw value
    range exceeds the 4 KiB stage although k_facts sees an empty value and the block fails emit_fast."""
    b = E.t_batch(2, 16384, 4097, "middle", 0)
    f = E.facts(b, 2)
    at = int(np.nonzero(f["vraw"] == 4097)[0][0])
    assert f["vlen"][at] == 0 and f["vraw"][at] > E.STAGE_CAP and f["s_r"][at] <= E.PIECE_ROW_MAX
    r = E.route(b, O.encode_sst(b, O.params(block_size=16384)), 16)[1]
    assert _failing(r) and not r["huge"] and r["carry"]
    # and on a block of <= 64 rows and <= 4096 bytes, more than 256 value granules need such a tombstone
    b = E.t_batch(2, 4096, 4097, "middle", 0)
    r = E.route(b, O.encode_sst(b, O.params(block_size=4096)), 16)[1]
    assert _failing(r) == ["nv16"]


def test_f_lattice_placement():
    specs = E.f_specs()
    for c in E.F_LCPS:
        assert any(s[2] == c for s in specs)
    assert any(s[0] == s[1] == s[2] for s in specs) and any(s[2] == s[0] < s[1] for s in specs)
    assert {1, 2, 3} <= {s[1] for s in specs} and any(s[1] % 16 for s in specs)
    residues = [set() for _ in specs]
    edges = {1023: set(), 1024: set(), 2047: set(), 2048: set()}
    for rot in E.F_ROTATIONS:
        b, where = E.f_tiled(rot)
        assert b.n == E.F_N
        f = E.facts(b, 2)
        for e, si in where.items():
            assert (f["klen"][e - 1], f["klen"][e], f["lcp"][e]) == specs[si], (rot, e, specs[si])
            residues[si].add(e % 64)
            if e in edges:
                edges[e].add(si)
        ref = O.encode_sst(b, O.params())
        assert ref.status == 0
    for si, r in enumerate(residues):
        assert {0, 1, 63} <= r, (specs[si], sorted(r))
    # lane 63 / lane 0 of a thread's second entry (1023 / 1024) and of the next workgroup (2047 / 2048)
    assert all(edges.values()), edges
    assert len(E.f_lattice_cases()) == len(E.F_ROTATIONS) * 4


def test_f_tails_geometry_and_errors():
    tails = E.f_tail_cases()
    assert len(tails) == 8 * 2
    for c in tails:
        b = c.batch
        k = c.expect["short"]
        assert int(b.key_off[b.n] - b.key_off[b.n - k]) < 16, c.name
        if "lane0" in c.name:
            assert (b.n - 1) % 64 == 0 and int(b.key_off[b.n] - b.key_off[b.n - 2]) < 16 <= int(b.key_off[b.n - 2])
        assert c.ref().status == 0, c.name
    geo = E.f_geometry_cases()
    assert sorted({c.expect["n"] for c in geo}) == list(E.F_GEOMETRY_N) and len(geo) == 10
    for c in geo:
        ref = c.ref()
        assert ref.status == 0 and c.batch.n == c.expect["n"]
        image, pieces, workgroup = E.counts(c.routes(ref))
        assert (pieces, workgroup) == (0, 0), c.name
        if c.kw["block_size"] == 64:
            assert ref.summary.num_blocks == image == c.batch.n, c.name  # every entry its own block
    errs = E.f_error_cases()
    assert len(errs) == len(E.F_ERRORS) * 3 + 2 + 2
    for c in errs:
        ref = c.ref()
        assert c.batch.n == E.F_ERR_N
        assert ref.status == c.expect["status"], (c.name, ref.status)
        if ref.status:
            assert ref.summary.first_error_entry == c.expect["entry"], c.name
    assert {c.expect["entry"] // E.CHUNK for c in errs if c.expect["entry"]} == {0, 1}


def test_c_cases_straddle_the_lookahead():
    cases = E.c_cases()
    assert len(cases) == len(E.c_block_sizes(2)) + len(E.c_block_sizes(1)) == 6 + 7
    for c in cases:
        bs, x = c.kw["block_size"], c.expect
        ref = c.ref()
        assert ref.status == 0 and ref.summary.max_block_entries <= x["wmax"], c.name
        assert x["mode"] == (1 if x["wmax"] <= E.seg_look(bs) else 0)
    assert E.seg_look(12252) == E.SEG_LOOK - 1 and E.seg_look(12264) == E.SEG_LOOK
    for v in (2, 1):
        by = {c.kw["block_size"]: c for c in cases if c.version == v}
        t = E.c_threshold(v)
        assert by[t - 1].expect == dict(wmax=E.SEG_LOOK, mode=1) and by[t].expect["mode"] == 0, (v, t)
        assert by[t].expect["wmax"] in (E.SEG_LOOK + 1, E.SEG_LOOK + 2)
        assert by[8192].expect["mode"] == by[12252].expect["mode"] == by[12264].expect["mode"] == 1
        serial = by[E.C_SERIAL_BS[v]]
        assert E.SEG_LOOK < serial.expect["wmax"] < E.CHUNK and serial.expect["mode"] == 0
        first = serial.ref().block_first_entry
        assert any(int(s) < E.CHUNK < int(e) for s, e in zip(first[:-1], first[1:]))  # a block straddles entry 2048


def test_longest_candidate_is_the_oracle_from_every_start():
    """A candidate block from entry s is the first block of the batch that starts at s."""
    b = E.tiny_rows(300)
    for v, ri in E.FORMATS:
        prm = O.params(block_size=1000, sst_version=v, restart_interval=ri, bloom_bits_per_key=0)
        want = max(int(O.encode_sst(b.slice(s, b.n), prm).block_first_entry[1]) for s in range(b.n))
        assert E.longest_candidate(b, v, 1000, ri) == want, (v, ri)


def test_longest_candidate_bounds_the_oracle():
    """The restated candidate length is the oracle's longest block when every candidate is a block start."""
    b = E.tiny_rows(700)
    for v, ri in E.FORMATS:
        for bs in (64, 100, 1000):
            ref = O.encode_sst(b, O.params(block_size=bs, sst_version=v, restart_interval=ri))
            w = E.longest_candidate(b, v, bs, ri)
            assert ref.summary.max_block_entries <= w <= bs // 12 + 1
            # uniform rows: a candidate is at most one restart row (3 bytes dearer than the others) or one
            # shorter shared prefix away from an actual block
            assert w - ref.summary.max_block_entries <= 1, (v, ri, bs, w, ref.summary.max_block_entries)


def test_p_shapes_take_their_chain_paths():
    """The shapes the GPU tests use for k_anchor's streamed tables and k_group's HBM compose take those
    paths by the kernels' predicates, and the oracle accepts them."""
    b = E.tiny_rows(E.P_STREAMED_N)
    for bs in E.P_STREAMED_BS:
        w = E.longest_candidate(b, 2, bs, 16)
        assert E.anchor_path(b.n, w, bs) == "streamed", (bs, w)
        assert O.encode_sst(b, O.params(block_size=bs)).status == 0
    b = E.tiny_rows(E.P_CUTS_N)
    w = E.longest_candidate(b, 2, E.P_CUTS_BS, 16)
    k, g, ng = E.chain_geometry(b.n)
    assert (k, g, ng) == (34, 16, 3) and E.group_paths(b.n, w, E.P_CUTS_BS) == {"hbm", "lds"}, w
    assert [min(g, k - q * g) * w * 14 + 64 > E.GROUP_LDS for q in range(ng)] == [True, True, False]
    # the chain enters groups 1 and 2 at candidates other than 0, after byte0 / byte1 bytes: the cut sizes sit
    # around them, so the walk takes group 0's table, then also group 1's, and cuts inside the next group
    ref = O.encode_sst(b, O.params(block_size=E.P_CUTS_BS))
    at = [int(np.searchsorted(ref.block_first_entry, q * g * E.CHUNK)) for q in (1, 2)]
    (o1, byte0), (o2, byte1) = [(int(ref.block_first_entry[i]) - q * g * E.CHUNK, int(ref.block_off[i]))
                                for q, i in zip((1, 2), at)]
    assert 0 < o1 < w and 0 < o2 < w
    small, behind, inside, both, one = E.P_CUTS_MAX_SST
    # (byte1 is what group 0's and group 1's tables add up to: past `inside`, within `both`)
    assert small < byte0 <= behind < inside < byte1 <= both < ref.summary.data_len < one
    cuts = {m: O.sst_cuts(b, O.params(block_size=E.P_CUTS_BS), m) for m in E.P_CUTS_MAX_SST}
    assert all(st == 0 for st, _ in cuts.values())
    assert len(cuts[small][1]) > 20 and cuts[one][1] == [0, b.n]
    first = lambda m: cuts[m][1][1]
    assert g * E.CHUNK + o1 <= first(behind) < first(inside) < 2 * g * E.CHUNK  # the first cut lies in group 1
    assert 2 * g * E.CHUNK + o2 <= first(both) < b.n  # ... in group 2
    # the neighbours of the streamed window, and the serial walk
    assert E.anchor_path(E.P_STREAMED_N, 100, 4096) == "lds" and E.anchor_path(E.P_STREAMED_N, 200, 4096) == "hbm"
    assert E.anchor_path(E.C_N, E.SEG_LOOK + 1, 16384) == "mode0"
    assert E.group_paths(E.C_N, E.SEG_LOOK + 1, 16384) == {"mode0"}
