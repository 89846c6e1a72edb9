"""f3 write side at its edges: sdb_compress_blocks on the adversarial payloads of tests/codec_payloads.py
(skewed histograms, mixes of compressible / constant / incompressible windows, sequence stress, degenerate
sizes), every codec, one compress launch per codec.

Every block must carry the CRC of its compressed bytes, stay within the literal-only bound its slot counts
on, declare its length, and decode to the input through the canonical library, the oracle, the device's
two-step decompressor and its decode-once path.  Then the witnesses: O.stream_stats of the device's own
streams proves that the branches the payloads aim at ran (which deflate / zstd block kinds, literal and
sequence table modes, repeat offsets, length extensions, element kinds), so a change of the encoder that
stops reaching one fails here instead of going untested.

Witnesses this encoder cannot show, by construction (each is asserted absent, so a change that makes one
reachable is noticed):
  * a 15-bit deflate literal / length or distance code from the length limit: a deflate block codes one
    4 KiB window, at most 4097 symbols, and only 4180 force a code deeper than 15
    (codec_payloads.fibonacci_payload, test_codec_payloads.test_huffman_depths);
  * zstd RLE literals inside a compressed block: every byte value first appears as a literal, so one-valued
    literals mean a constant window, which is an RLE block; treeless literals and the repeat table mode are
    never written; the 5-byte literals header needs more than 16383 literals, a window has 4096;
  * lz4 match-length extensions of 2 or more bytes: a window's longest match is 258 bytes (kCzMaxMatch),
    258 - 4 - 15 < 255: one extension byte.
"""
import struct
import zlib

import numpy as np
import pytest

from oracle import oracle as O

from . import codec_payloads as P
from .test_gpu_codec_once import NONE, _check
from .test_gpu_codec_write import CODECS, canonical_decompress, compressed_on_device
from .test_gpu_parity import rt  # noqa: F401

pytestmark = pytest.mark.gpu

_cache = {}


class Run:
    """The payload list compressed on the device by one codec: the streams, and their stats."""

    def __init__(self, rt, codec):  # noqa: F811
        self.codec = codec
        self.payloads = P.payload_list()
        self.data, self.off = P.blocks_of(self.payloads)
        self.comp, self.coff = compressed_on_device(rt, codec, self.data, self.off)
        self.nb = len(self.payloads)
        assert len(self.coff) == self.nb + 1
        self.streams = [self.comp[int(self.coff[k]):int(self.coff[k + 1]) - 4].tobytes() for k in range(self.nb)]
        self.stats = [O.stream_stats(codec, s) for s in self.streams]
        self.ref = O.decompress_blocks(codec, self.comp, self.coff)

    def where(self, pred):
        """The names of the payloads whose (name, payload, stats) satisfy pred."""
        return [n for (n, p), s in zip(self.payloads, self.stats) if pred(n, p, s)]


def run_of(rt, codec):  # noqa: F811
    if codec not in _cache:
        _cache[codec] = Run(rt, codec)
    return _cache[codec]


def bound(codec, n):
    """The literal-only worst case the slot layout counts on (sdb_codec_enc.hip, cz_slot), CRC included."""
    w = max(1, -(-n // P.WIN))
    return {O.CODEC_LZ4: n + n // 255 + 10, O.CODEC_SNAPPY: n + 14, O.CODEC_ZLIB: n + 5 * w + 6,
            O.CODEC_ZSTD: n + 3 * w + 12}[codec] + 4


def declared_length(codec, stream, stats):
    if codec == O.CODEC_LZ4:
        return struct.unpack("<I", stream[:4])[0]
    if codec == O.CODEC_SNAPPY:
        v, i = 0, 0
        while True:
            v |= (stream[i] & 0x7F) << (7 * i)
            if not stream[i] & 0x80:
                return v
            i += 1
    if codec == O.CODEC_ZSTD:
        assert stats["zs_fcs_bytes"] in (1, 2, 4)
        return stats["zs_fcs"]
    return None  # zlib declares none


@pytest.mark.parametrize("codec", CODECS)
def test_edge_blocks_are_valid_streams(rt, codec):  # noqa: F811
    r = run_of(rt, codec)
    assert r.coff[0] == 0 and np.all(np.diff(r.coff.astype(np.int64)) > 4)  # monotone: a stream and its CRC
    assert r.ref.status == 0 and r.ref.first_err == NONE, (r.ref.status, hex(r.ref.first_err))
    for k, (name, p) in enumerate(r.payloads):
        n = len(p)
        blk = r.comp[int(r.coff[k]):int(r.coff[k + 1])].tobytes()
        stream, st = r.streams[k], r.stats[k]
        assert struct.unpack(">I", blk[-4:])[0] == zlib.crc32(stream), (name, codec)
        assert len(blk) <= bound(codec, n), (name, codec, n, len(blk), bound(codec, n))
        d = declared_length(codec, stream, st)
        assert d is None or d == n, (name, codec, d, n)
        assert canonical_decompress(codec, stream, n) == p, (name, codec)
        assert st["status"] == 0, (name, codec)
        a, b = int(r.ref.out_start[k]), int(r.ref.out_end[k])
        assert b - a == n + 4 and r.ref.out[a:b - 4].tobytes() == p, (name, codec)
        assert struct.unpack(">I", r.ref.out[b - 4:b].tobytes())[0] == zlib.crc32(p), (name, codec)


@pytest.mark.parametrize("codec", CODECS)
def test_edge_blocks_decode_on_device(rt, codec):  # noqa: F811
    import torch
    r = run_of(rt, codec)
    blocks = torch.from_numpy(np.concatenate([r.comp, np.zeros(64, np.uint8)])).cuda()
    boff = torch.from_numpy(r.coff.view(np.int64)).cuda()
    out, out_start, out_end, err = rt.decompress_blocks_device(codec, blocks, boff)
    torch.cuda.synchronize()
    assert int(err.cpu().numpy().view(np.uint64)[0]) == r.ref.first_err == NONE
    start, end = out_start.cpu().numpy().view(np.uint64), out_end.cpu().numpy().view(np.uint64)
    assert np.array_equal(start, r.ref.out_start) and np.array_equal(end, r.ref.out_end)
    got = out.cpu().numpy()
    for k, (name, p) in enumerate(r.payloads):
        assert got[int(start[k]):int(end[k]) - 4].tobytes() == p, (name, codec)
    # decode-once at a slot every block fits and at one none does (out_start / out_end / err against the
    # oracle's inside _check; zlib's slots make its out_start its own, the lengths are the oracle's)
    comp = np.concatenate([r.comp, np.zeros(64, np.uint8)])
    fit = (max(len(p) for _, p in r.payloads) + 4 + 15) & ~7
    for slot in (fit, 8):
        o, s, e, er, spilled = _check(codec, comp, r.coff, slot)
        assert er == NONE
        if codec == O.CODEC_ZLIB:
            assert spilled == (0 if slot == fit else sum(len(p) + 4 > 8 for _, p in r.payloads))
        for k, (name, p) in enumerate(r.payloads):
            assert o[int(s[k]):int(e[k]) - 4].tobytes() == p, (name, codec, slot)


def witness(r, what, pred):
    names = r.where(pred)
    print("witness %-9s %-58s %s" % ({1: "snappy", 2: "zlib", 3: "lz4", 4: "zstd"}[r.codec], what, names[:4]))
    return names


def test_witnesses_zlib(rt):  # noqa: F811
    r = run_of(rt, O.CODEC_ZLIB)
    missing = []

    def need(what, pred):
        if not witness(r, what, pred):
            missing.append(what)

    need("a stored block", lambda n, p, s: s["kinds"][0])
    need("a fixed block", lambda n, p, s: s["kinds"][1])
    need("a dynamic block", lambda n, p, s: s["kinds"][2])
    need("stored, fixed and dynamic blocks in one stream", lambda n, p, s: all(s["kinds"]))
    need("a dynamic block after a first block that is not", lambda n, p, s: s["blocks"][0] != 2 and 2 in s["blocks"][1:])
    need("a fixed block after a partial byte of a dynamic one", lambda n, p, s: (2, 1) in zip(s["blocks"], s["blocks"][1:]))
    need("a match of 258 bytes", lambda n, p, s: s["max_match"] == 258)
    # (the far-offset payloads are random bytes around one match: deflate stores them; far matches are
    # witnessed where the window also compresses)
    for off in (1, 2, 3):
        need("a match at distance %d" % off, lambda n, p, s: n == "offset-%d" % off and s["max_dist"] == off)
    need("a match at a distance of 2048 or more", lambda n, p, s: s["max_dist"] >= 2048)
    need("a match at a distance of 4000 or more", lambda n, p, s: s["max_dist"] >= 4000)
    need("the lazy step: one 12-byte match, none of 4", lambda n, p, s: n == "lazy" and s["matches"] == 1
         and s["max_match"] == 12)
    need("a window of about a thousand sequences", lambda n, p, s: s["nblocks"] == 1 and s["matches"] >= 800)
    need("a 7-bit code-length code where the histogram needs 8", lambda n, p, s: s["z_max_cl_len"] == 7
         and P.huffman_depth(s["z_cl_hist"]) > 7)
    assert not missing, missing
    # one deflate block per window, and the length limit out of reach (see the module docstring): every
    # dynamic block codes at most a window + end-of-block, so no histogram forces a code past 15 bits
    for (name, p), s in zip(r.payloads, r.stats):
        assert s["nblocks"] == max(1, -(-len(p) // P.WIN)), name
        assert s["z_max_ll_len"] <= 15 and s["z_max_d_len"] <= 15 and s["z_max_cl_len"] <= 7, name
        total = sum(s["z_ll_hist"])
        assert total <= P.WIN + 1 < P.min_total_for_depth(16), name
        if total:
            print("zlib depth %-28s declared %2d, least optimal %2d, code-length code %d" %
                  (name, s["z_max_ll_len"], P.huffman_depth(s["z_ll_hist"]), s["z_max_cl_len"]))


def test_witnesses_zstd(rt):  # noqa: F811
    r = run_of(rt, O.CODEC_ZSTD)
    missing = []

    def need(what, pred):
        if not witness(r, what, pred):
            missing.append(what)

    need("raw, RLE and compressed blocks in one frame", lambda n, p, s: all(s["kinds"]))
    need("Huffman literals in 1 stream", lambda n, p, s: s["zs_lit_streams"][0])
    need("Huffman literals in 4 streams, 3-byte header", lambda n, p, s: s["zs_lit_sizefmt"][1])
    need("Huffman literals in 4 streams, 4-byte header", lambda n, p, s: s["zs_lit_sizefmt"][2])
    need("raw literals inside a compressed block", lambda n, p, s: n == "random-then-copy" and s["zs_lit_type"][0]
         and s["kinds"] == [0, 0, 1] and s["zs_nseq"])
    need("a direct tree description", lambda n, p, s: s["zs_huf_direct"])
    need("an FSE-compressed tree description", lambda n, p, s: s["zs_huf_fse"])
    need("an FSE-compressed tree description over 128 weights", lambda n, p, s: n == "wide-skewed" and s["zs_huf_fse"])
    need("an 11-bit code on literals that need a deeper one", lambda n, p, s: s["zs_huf_maxbits"] == 11
         and P.huffman_depth(s["zs_lit_hist"]) > 11)
    for t, table in enumerate(("LL", "OF", "ML")):
        for m, mode in enumerate(("predefined", "RLE", "FSE")):
            need("%s table %s" % (table, mode), lambda n, p, s: s["zs_mode"][t][m])
    need("a repeat-offset sequence", lambda n, p, s: s["zs_rep"])
    need("a repeat-offset sequence with ll == 0", lambda n, p, s: s["zs_rep_ll0"])
    need("a repeat offset in a window after a raw window", lambda n, p, s: s["zs_rep_after_raw"])
    need("the carried repeat offset after a discarded window", lambda n, p, s: n.startswith("mix-rep-carry")
         and s["blocks"][:3] == [2, 0, 2] and s["zs_rep_after_raw"])
    for nbytes in (1, 2, 4):
        need("frame header with a %d-byte content size" % nbytes, lambda n, p, s: s["zs_fcs_bytes"] == nbytes)
    need("a window of about a thousand sequences", lambda n, p, s: s["nblocks"] == 1 and s["zs_nseq"] >= 800)
    assert not missing, missing
    for (name, p), s in zip(r.payloads, r.stats):
        assert s["nblocks"] == max(1, -(-len(p) // P.WIN)), name
        assert s["zs_lit_type"][1] == s["zs_lit_type"][3] == 0 and s["zs_lit_sizefmt"][3] == 0, name
        assert all(m[3] == 0 for m in s["zs_mode"]) and s["zs_huf_maxbits"] <= 11, name
        assert (s["zs_fcs_bytes"] == 1) == (len(p) < 256) and (s["zs_fcs_bytes"] == 4) == (len(p) >= 65792), name
        if len(p) < 16 and len(set(p)) > 1:
            assert s["blocks"] == [0], name  # under 16 bytes the compressor is skipped


def test_witnesses_lz4(rt):  # noqa: F811
    r = run_of(rt, O.CODEC_LZ4)
    missing = []

    def need(what, pred):
        if not witness(r, what, pred):
            missing.append(what)

    need("a literal length extension of 2 bytes", lambda n, p, s: s["lz_max_lit_ext"] == 2)
    need("a literal length extension of 3 or more bytes", lambda n, p, s: s["lz_max_lit_ext"] >= 3 and s["matches"])
    need("a match length extension byte", lambda n, p, s: s["lz_max_match_ext"] == 1)
    need("a block over 4 KiB on the multi-window path", lambda n, p, s: len(p) > P.WIN and s["matches"]
         and s["lz_last_match_pos"] >= P.WIN)
    need("a block over 4 KiB on the literal-only fallback", lambda n, p, s: len(p) > P.WIN and not s["matches"]
         and s["lz_elems"] == 1)
    assert not missing, missing
    by = {n: s for (n, _), s in zip(r.payloads, r.stats)}
    # literal runs around the extension steps 15 and 15 + 255: exactly the bytes the format needs
    for n in P.LITERAL_RUNS:
        s = by["litrun-%d" % n]
        assert s["matches"] == 1 and s["max_match"] == 8 and s["max_dist"] == n, n
        assert s["lz_max_lit_ext"] == (0 if n < 15 else (n - 15) // 255 + 1), (n, s["lz_max_lit_ext"])
    for n in P.MATCH_LENGTHS:
        s = by["match-%d" % n]
        assert s["max_match"] == min(n, 258) and s["matches"] == (1 if n < 258 + 4 else 2), (n, s["matches"])
        assert s["lz_max_match_ext"] == (min(n, 258) - 4 >= 15), n
    # the end rules: a match starts 12+ bytes before the end of the block and ends 5+ before it
    for g, t in P.END_MATCHES:
        s = by["endmatch-%d-%d" % (g, t)]
        want = P.lz4_end_rule_length(g, t)
        assert s["matches"] == (want > 0) and s["max_match"] == want, (g, t, s["matches"], s["max_match"], want)
    for (name, p), s in zip(r.payloads, r.stats):
        assert s["lz_max_match_ext"] <= 1 and s["max_match"] <= 258, name  # kCzMaxMatch: see the module docstring


def test_witnesses_snappy(rt):  # noqa: F811
    r = run_of(rt, O.CODEC_SNAPPY)
    missing = []

    def need(what, pred):
        if not witness(r, what, pred):
            missing.append(what)

    need("a copy-1 element", lambda n, p, s: s["sn_tag"][1])
    need("a copy-2 element", lambda n, p, s: s["sn_tag"][2])
    need("a match split into chunks of 64", lambda n, p, s: s["sn_split64"])
    need("a match split into 60 and the rest", lambda n, p, s: s["sn_split60"])
    for nbytes in (1, 2, 3):
        need("a literal with a %d-byte tag" % nbytes, lambda n, p, s: s["sn_lit_tag_bytes"][nbytes])
    need("the literal-only stream where elements would be longer", lambda n, p, s: len(p) > P.WIN and s["lz_elems"] == 1
         and s["sn_tag"][0] == 1)
    assert not missing, missing
    by = {n: s for (n, _), s in zip(r.payloads, r.stats)}
    # an 8-byte match is a copy-1 element below offset 2048 and a copy-2 element from there on; 40 bytes
    # are copy-2 at any offset
    assert by["offset8-2047"]["sn_tag"][1:3] == [1, 0] and by["offset8-2048"]["sn_tag"][1:3] == [0, 1]
    assert by["offset-3"]["sn_tag"][1:3] == [0, 1] and by["offset-2047"]["sn_tag"][1:3] == [0, 1]
    # literal tags: the length in the tag up to 60 bytes, one length byte up to 256, then two
    for n in P.LITERAL_RUNS:
        s = by["litrun-%d" % n]
        tag = 1 if n <= 60 else 2 if n <= 256 else 3
        assert s["matches"] == 1 and s["sn_lit_tag_bytes"][tag] >= 1 and s["sn_tag"][0] == 2, (n, s["sn_lit_tag_bytes"])
        assert sum(s["sn_lit_tag_bytes"]) == s["sn_lit_tag_bytes"][tag] + (tag != 1), n  # and the 14-byte tail
    # a match of 258 bytes: 64 + 64 + 64 + 60 + 6; of 64, 65..67, 68 bytes: whole, 60 + rest, 64 + rest
    s = by["match-258"]
    assert s["matches"] == 5 and s["sn_split64"] == 3 and s["sn_split60"] == 1 and s["sn_tag"][1] == 1
    for (name, p), s in zip(r.payloads, r.stats):
        assert s["sn_tag"][3] == 0 and s["max_match"] <= 64, name
