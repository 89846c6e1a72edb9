"""CPU pins for the test infrastructure of the write-side edge tests: O.stream_stats (the oracle's
decompressors counting what a stream is made of) against streams whose structure is known, and the
properties of the adversarial payload generators (tests/codec_payloads.py) that belong to the input."""
import struct
import zlib
from collections import Counter

import numpy as np
import pytest

from oracle import oracle as O

from . import codec_payloads as P
from .test_codec_entropy import frame as zstd_frame
from .test_codec_entropy import payloads

pa = pytest.importorskip("pyarrow")

TEXT = b"".join(b"key%06d=value-%d;" % (i, i * i % 97) for i in range(3000))


def zl(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return c.compress(data) + c.flush()


# ------------------------------------------------------------------------------------------------
# stream_stats
# ------------------------------------------------------------------------------------------------
def test_stats_zlib_block_kinds():
    for p in payloads():
        s = O.stream_stats(O.CODEC_ZLIB, zl(p, 0))
        assert s["status"] == 0 and s["kinds"][1] == s["kinds"][2] == 0 and s["kinds"][0] >= 1, len(p)
        assert s["kinds"][0] == s["nblocks"] >= -(-len(p) // 65535) and s["matches"] == 0
        assert s["blocks"] == [0] * min(s["nblocks"], 64)
        s = O.stream_stats(O.CODEC_ZLIB, zl(p, 6, zlib.Z_FIXED))
        assert s["status"] == 0 and s["kinds"][0] == s["kinds"][2] == 0 and s["kinds"][1] >= 1, len(p)
        assert s["z_max_ll_len"] == s["z_max_cl_len"] == 0  # only dynamic blocks have code lengths of their own
    for p in (TEXT, payloads()[0]):
        s = O.stream_stats(O.CODEC_ZLIB, zl(p, 6, zlib.Z_HUFFMAN_ONLY))
        assert s["status"] == 0 and s["kinds"][2] >= 1 and s["kinds"][0] == 0 and s["matches"] == 0
        assert 1 <= s["z_max_ll_len"] <= 15 and 1 <= s["z_max_cl_len"] <= 7 and s["max_match"] == 0


def test_stats_zlib_matches_and_histogram():
    s = O.stream_stats(O.CODEC_ZLIB, zl(TEXT))
    assert s["blocks"] == [2] and 0 < s["matches"] and 3 <= s["max_match"] <= 258 and 0 < s["max_dist"] <= 32768
    h = s["z_ll_hist"]
    assert h[256] == 1 and sum(h[257:]) == s["matches"] and sum(h[:256]) > 0
    # the longest code the histogram needs is no longer than the one the stream declares
    assert P.huffman_depth(h) <= s["z_max_ll_len"] <= 15
    run = O.stream_stats(O.CODEC_ZLIB, zl(bytes(5000)))
    assert run["max_match"] == 258 and run["max_dist"] == 1
    # a sync flush: an empty stored block between two dynamic ones, in order
    c = zlib.compressobj(6)
    z = c.compress(TEXT[:20000]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(TEXT[20000:]) + c.flush()
    assert O.stream_stats(O.CODEC_ZLIB, z)["blocks"] == [2, 0, 2]


def test_stats_zstd_hand_built_frames():
    raw = (0, b"hello world", b"hello world")
    rle = (1, bytes([0x41, 200]), b"A" * 200)
    s = O.stream_stats(O.CODEC_ZSTD, zstd_frame([raw, rle], checksum=True))
    assert s["status"] == 0 and s["blocks"] == [0, 1] and s["kinds"] == [1, 1, 0]
    assert s["zs_fcs_bytes"] == 4 and s["zs_fcs"] == 211 and s["zs_nseq"] == 0 and sum(s["zs_lit_type"]) == 0
    s = O.stream_stats(O.CODEC_ZSTD, zstd_frame([rle, raw, rle]))
    assert s["blocks"] == [1, 0, 1]


def test_stats_zstd_library_streams():
    seen_huf = 0
    for p in payloads():
        z = pa.Codec("zstd", compression_level=3).compress(p, asbytes=True)
        s = O.stream_stats(O.CODEC_ZSTD, z)
        assert s["status"] == 0 and s["zs_fcs"] == len(p), len(p)
        assert s["zs_fcs_bytes"] == (1 if len(p) < 256 else 2 if len(p) < 65792 else 4)
        assert s["zs_rep_ll0"] <= s["zs_rep"] <= s["zs_nseq"] == s["matches"]
        assert sum(s["zs_lit_type"]) == s["kinds"][2]
        seen_huf += s["zs_lit_type"][2]
    assert seen_huf
    s = O.stream_stats(O.CODEC_ZSTD, pa.Codec("zstd", compression_level=3).compress(TEXT, asbytes=True))
    assert s["blocks"] == [2] and s["zs_lit_type"][2] == 1 and s["zs_lit_streams"] == [0, 1]
    assert s["zs_huf_direct"] + s["zs_huf_fse"] == 1 and 1 <= s["zs_huf_maxbits"] <= 11
    assert sum(s["zs_lit_hist"]) > 0 and P.huffman_depth(s["zs_lit_hist"]) <= s["zs_huf_maxbits"]
    assert [sum(m) for m in s["zs_mode"]] == [1, 1, 1] and s["zs_rep"] > 0


def test_stats_lz4_snappy_extensions():
    data = bytes(np.random.default_rng(5).integers(0, 256, 1000, dtype=np.uint8)) + bytes(5000) + b"tail-bytes!!"
    z = struct.pack("<I", len(data)) + pa.compress(data, codec="lz4_raw", asbytes=True)
    s = O.stream_stats(O.CODEC_LZ4, z)
    assert s["status"] == 0 and s["matches"] >= 1 and s["lz_elems"] == s["matches"] + 1
    assert s["lz_max_lit_ext"] == (1000 - 15) // 255 + 1       # 1000 literals and a few of the run's bytes
    assert s["lz_max_match_ext"] >= (4990 - 19) // 255 + 1 and s["max_dist"] >= 1
    assert 1000 <= s["lz_last_match_pos"] < len(data)
    z = pa.compress(data, codec="snappy", asbytes=True)
    s = O.stream_stats(O.CODEC_SNAPPY, z)
    assert s["status"] == 0 and sum(s["sn_tag"]) == s["lz_elems"] and s["sn_tag"][0] >= 2
    assert s["sn_lit_tag_bytes"][3] >= 1 and s["sn_lit_tag_bytes"][1] >= 1  # 1000 literals: a 3-byte tag
    assert s["sn_split64"] >= 70 and s["max_match"] == 64                   # the run: copies of 64
    assert s["sn_tag"][1] + s["sn_tag"][2] + s["sn_tag"][3] == s["matches"]


def test_stats_leave_the_decode_alone():
    """The sink is optional: the bytes and the status with it equal those without it, errors included."""
    z = zl(TEXT)
    assert O.decompress(O.CODEC_ZLIB, z) == (0, TEXT)
    bad = bytearray(z)
    bad[-1] ^= 1
    assert O.stream_stats(O.CODEC_ZLIB, bytes(bad))["status"] == O.decompress(O.CODEC_ZLIB, bytes(bad))[0] != 0
    assert O.stream_stats(O.CODEC_ZSTD, b"\x28\xb5\x2f")["status"] != 0
    assert O.decompress(O.CODEC_ZLIB, z) == (0, TEXT)


# ------------------------------------------------------------------------------------------------
# the generators
# ------------------------------------------------------------------------------------------------
def test_generators_are_deterministic_and_named_once():
    a, b = P.payload_list(), P.payload_list()
    assert [n for n, _ in a] == [n for n, _ in b] and all(x[1] == y[1] for x, y in zip(a, b))
    assert len({n for n, _ in a}) == len(a)
    total = sum(len(p) for _, p in a)
    assert total < 1 << 20, total  # one launch per codec, under 1 MiB
    data, off = P.blocks_of(a)
    assert int(off[-1]) == len(data) == total + 4 * len(a)
    assert data[int(off[1]) - 4:int(off[1])].tobytes() == b"\xde\xad\xbe\xef"


def test_huffman_depths():
    """Fibonacci counts over 18 byte values need a code deeper than deflate's 15 bits, the 2^i counts one
    deeper than zstd's 11; and why no window can force deflate past 15."""
    by = dict(P.payload_list())
    for name in ("fib18-sorted", "fib18-shuffled"):
        c = Counter(by[name])
        assert len(c) == 18 and sorted(c.values()) == P.fibonacci_counts(18)
        assert P.huffman_depth(c.values()) == 17 > 15
    assert by["fib18-sorted"] == bytes(sorted(by["fib18-shuffled"])) != by["fib18-shuffled"]
    for name in ("fib16-sorted", "fib16-shuffled"):
        assert len(by[name]) == 2583 <= P.WIN and P.huffman_depth(Counter(by[name]).values()) == 15
    for name in ("pow2-sorted", "pow2-shuffled"):
        c = Counter(by[name])
        assert len(by[name]) == P.WIN and len(c) == 13 and P.huffman_depth(c.values()) == 12 > 11
    # the least histogram that forces depth d has Fibonacci counts; a deflate block of this encoder codes at
    # most 4096 literals / lengths + the end-of-block symbol
    assert P.min_total_for_depth(16) == 4180 > P.WIN + 1
    assert P.huffman_depth(P.fibonacci_counts(17)) == 16 and sum(P.fibonacci_counts(17)) == 4180
    f = P.fibonacci_counts(17)
    f[-1] -= 1  # one fewer: a tie, and the shallower tree wins it
    assert P.huffman_depth(f) == 15
    assert P.min_total_for_depth(12) == 609 <= P.WIN  # zstd's limit is within a window's reach
    assert P.min_total_for_depth(8) == 88             # the code-length code: 19 symbols, limit 7


def test_wide_skewed_alphabet():
    p = dict(P.payload_list())["wide-skewed"]
    c = Counter(p)
    assert len(p) == P.WIN and len(c) >= 200 and max(c) == 255
    assert max(c.values()) > 30 * min(c.values())
    assert P.huffman_depth(c.values()) > 11


def test_deep_literals_stay_literals():
    """Every 3-gram of the dictionary is distinct (no match inside it), every chain literal is followed by
    the first 3 bytes of a marker of its own (no 4 bytes from a chain literal on repeat), and the
    histogram of dictionary + chain forces a code deeper than 11."""
    p = P.deep_literals()
    n = sum(P.fibonacci_counts(P.DEEP_CHAIN))
    assert len(p) == n + 3 + 5 * n <= P.WIN
    d, rest = p[:n + 3], p[n + 3:]
    grams = [d[i:i + 3] for i in range(len(d) - 2)]
    assert len(set(grams)) == len(grams) and min(d) >= 16
    units = [rest[5 * i:5 * i + 5] for i in range(n)]
    assert all(u[0] < P.DEEP_CHAIN and u[1:] in d for u in units)
    assert len({u[1:4] for u in units}) == n
    counts = Counter(d) + Counter(u[0] for u in units)
    assert sorted(counts.values()) == sorted(P.deep_literal_counts())
    assert P.huffman_depth(counts.values()) > 11


def test_cl_limit_payload():
    """Every code for the payload's histogram has the planned lengths, their code-length sequence has no run
    to repeat, and the code-length code it needs is deeper than 7; zlib agrees (Z_HUFFMAN_ONLY: the same
    literals, no matches) and limits its code-length code to 7 too."""
    p = P.cl_limit_payload()
    lens = P.cl_limit_code_lengths()
    c = Counter(p)
    assert len(p) == 2047 and len(c) == 256 and all(c[v] == 2048 >> n for v, n in enumerate(lens))
    assert sum(2048 >> n for n in lens) + 1 == 2048            # dyadic with the end-of-block symbol
    assert len({p[i:i + 4] for i in range(len(p) - 3)}) == len(p) - 3
    assert all(not (lens[i] == lens[i + 1] == lens[i + 2] == lens[i + 3]) for i in range(253)) and lens[-1] == 11
    items = Counter(lens + [11] + [1, 1])                     # + end of block + two placeholder distance codes
    assert sorted(items.values()) == [2, 2, 3, 5, 8, 13, 21, 55, 150] and P.huffman_depth(items.values()) == 8 > 7
    s = O.stream_stats(O.CODEC_ZLIB, zl(p, 6, zlib.Z_HUFFMAN_ONLY))
    assert s["blocks"] == [2] and s["z_max_ll_len"] == 11 and s["z_max_cl_len"] == 7
    assert [s["z_cl_hist"][n] for n in range(4, 12)] == [3, 5, 8, 13, 21, 150, 55, 2]
    assert P.huffman_depth(s["z_cl_hist"]) > 7


def test_window_mixes():
    mixes = dict(P.window_mixes())
    assert sorted(len(p) for n, p in mixes.items() if n.startswith("mix-") and n[4].isdigit()) == sorted(P.MIX_SIZES)
    assert {4095, 4096, 4097, 8192, 12289, 65791, 65792, 65536 + 4} <= {len(p) for p in mixes.values()}
    # every kind stands first in a block, and follows every other kind class (compressible / constant / random)
    assert {o[0] for o in P.MIX_ORDERS} >= {"text", "rand", "const", "rand16"}
    p = mixes["mix-rep-carry"]
    assert p[:P.WIN] == p[2 * P.WIN:] and p[:700] == p[700:1400]           # the same period and bytes again
    mid = p[P.WIN:2 * P.WIN]
    assert len(set(mid)) == 256 and mid[3496:3500] == mid[2496:2500] and mid[3596:3600] == mid[1596:1600]
    p = mixes["mix-stored-dynamic-fixed"]
    assert len(p) == 2 * P.WIN + 17 and len(set(p[:P.WIN])) == 256 and max(p[P.WIN:2 * P.WIN]) < 128
    p = mixes["mix-rand-const-text"]
    assert len(set(p[P.WIN:2 * P.WIN])) == 1
    for kind, k in (("const", 1), ("rand4", 4), ("rand16", 16)):
        assert len(set(P.window_kind(kind, P.WIN, 3))) == k


def test_sequence_stress_shapes():
    by = dict(P.sequence_stress())
    g = by["grams-replay"]
    first = [g[4 * i:4 * i + 4] for i in range(455)]
    second = [g[1820 + 5 * i:1820 + 5 * i + 4] for i in range(455)]
    assert len(g) == 9 * 455 <= P.WIN and len(set(first)) == 455 and sorted(first) == sorted(second) and first != second
    all4 = [g[i:i + 4] for i in range(1820 - 3)]
    assert len(set(all4)) == len(all4)  # no match inside the first part
    d = by["grams-dictionary"]
    assert len(d) == P.WIN and len({d[4 * i:4 * i + 4] for i in range(64)}) == 64
    assert all(d[256 + 4 * i:260 + 4 * i] in d[:256] for i in range(960))
    # the matches below are where the single-probe finders (lz4 / snappy) look: no hash collision between
    for n in P.MATCH_LENGTHS:
        p = by["match-%d" % n]
        src = max(300, n)
        assert p[src + 20:src + 20 + n] == p[:n] and p[src + 20 + n] != p[n]
        assert P.single_probe_source(p, src + 20) == 0
    for n in P.LITERAL_RUNS:
        p = by["litrun-%d" % n]
        assert p[n:n + 8] == p[:8] and p[n + 8] != p[8] and len(p) == n + 22 <= P.WIN
        assert P.single_probe_source(p, n) == 0
    for off in P.OFFSETS:
        p = by["offset-%d" % off]
        at = 24 + off if off <= 3 else off
        assert p[at:at + 40] == p[at - off:at - off + 40] and len(p) <= P.WIN
        assert off <= 3 or P.single_probe_source(p, at) == 0
    for off in P.SHORT_OFFSETS:
        p = by["offset8-%d" % off]
        assert p[off:off + 8] == p[:8] and p[off + 8] != p[8] and P.single_probe_source(p, off) == 0
    for g, t in P.END_MATCHES:
        p = by["endmatch-%d-%d" % (g, t)]
        assert p[g + 30:2 * g + 30] == p[:g] and len(p) == 2 * g + 30 + t and P.single_probe_source(p, g + 30) == 0
    assert [P.lz4_end_rule_length(8, t) for t in (0, 1, 3, 4, 5, 6)] == [0, 0, 0, 7, 8, 8]
    assert [P.lz4_end_rule_length(16, t) for t in (0, 1, 4, 5, 6)] == [11, 12, 15, 16, 16]
    p = by["lazy"]
    q = P.LAZY_AT
    assert p[q:q + 4] == p[:4] and p[q + 4] != p[4]                 # 4 bytes at q, no more
    assert p[q + 1:q + 13] == p[24:36] and p[q + 13] != p[36]       # 12 bytes at q + 1
    assert P.single_probe_source(p, q) == 0 and P.single_probe_source(p, q + 1) == 24


def test_degenerate_sizes_and_alphabets():
    d = P.degenerate()
    lens = [len(p) for n, p in d if n.startswith("len-")]
    assert lens == [0, 1, 2, 3, 4, 5, 12, 13, 15, 16, 63, 64, 65, 127, 128, 255, 256, 16383, 16384]
    tiny = [len(p) for n, p in d if n.startswith("tiny-")]
    assert tiny == [k % 7 for k in range(300)]
    names = [n for n, _ in d]
    k0 = names.index("tiny-000")
    assert names[k0:k0 + 300] == ["tiny-%03d" % k for k in range(300)]  # consecutive: adjacent slots
    by = dict(d)
    assert all(len(set(p)) == 1 for n, p in d if n.startswith("one-symbol"))
    assert all(len(set(p)) == 2 for n, p in d if n.startswith("two-symbols"))
    assert len(by["one-symbol-%d" % P.WIN]) == P.WIN
