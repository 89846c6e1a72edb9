"""f3 on the device: which status a bad block gets, and which of a run's bad blocks the error word names.

decode_block's frame rules (format/sst.rs:980-999), in their order of precedence: a block too short for its
CRC -> SDB_CORRUPT_BLOCK; the stored CRC (validate_checksum) -> SDB_CHECKSUM_MISMATCH, whatever the payload
holds; a header the plan cannot size -> SDB_DECOMPRESSION_ERROR, or SDB_LIMIT_EXCEEDED when it declares more
than 64 MiB (LZ4 / Snappy: the entropy codecs declare nothing); then the payload's own decode.  The error word
is the minimum of block << 8 | status over the run's blocks, not the last one written.

Every case is a run [good, BAD, good] of blocks of a few hundred bytes, plus one run of all the bad blocks in
order and the same run reversed, through sdb_decompress_plan + sdb_decompress_blocks and through
sdb_decompress_blocks_once (at a slot every good block overflows and one it fits): the error word, every
block's length and every block's bytes equal the oracle's."""
import functools
import struct

import numpy as np
import pytest

from oracle import oracle as O
from slatedb_amd import _abi

from .codec_util import compress_payload, frame
from .test_gpu_codec import _check as check_run
from .test_gpu_codec_once import _check as check_once

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

CODECS = [O.CODEC_LZ4, O.CODEC_SNAPPY, O.CODEC_ZLIB, O.CODEC_ZSTD]
LZ = (O.CODEC_LZ4, O.CODEC_SNAPPY)
NONE = 2**64 - 1
OVER = (64 << 20) + 1


def _varint(v):
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def _declare(codec, n, body):
    """An LZ4 / Snappy payload whose header declares n bytes."""
    return (struct.pack("<I", n) if codec == O.CODEC_LZ4 else _varint(n)) + body


def _flip(block, at, bit=0x10):
    b = bytearray(block)
    b[at] ^= bit
    return bytes(b)


def _bad_blocks(codec):
    """(name, stored block) for every kind of bad block that applies to the codec."""
    raw = b"".join(b"key%04d=value-%d;" % (i, i * i % 97) for i in range(16))[:256]
    good = compress_payload(codec, raw)
    junk = bytes((37 * i + 11) & 0xFF for i in range(48))
    garbage = _declare(codec, 200, junk) if codec in LZ else junk  # a readable length, then no valid stream
    bad = [("empty", b""), ("short", b"\x01\x02\x03"), ("garbage", frame(garbage)),
           ("garbage-crc", _flip(frame(garbage), len(garbage) + 1)), ("cut", frame(good[:-7]))]
    if codec == O.CODEC_ZLIB:
        bad.append(("adler", frame(_flip(good, len(good) - 1, 0x01))))
    if codec in LZ:
        bad.append(("over-64MiB", frame(_declare(codec, OVER, junk))))
        bad.append(("no-length", frame(b"\xff" * 5 if codec == O.CODEC_SNAPPY else b"\x01\x02")))
    return bad


def _run_of(blocks):
    return (np.frombuffer(b"".join(blocks), np.uint8).copy(),
            np.cumsum([0] + [len(b) for b in blocks]).astype(np.uint64))


@functools.lru_cache(maxsize=None)
def _runs(codec):
    """[(name, comp, coff)]: [good, BAD, good] per bad block, then all of them in order and reversed."""
    g0 = frame(compress_payload(codec, bytes(range(200)) + b"tail" * 11))
    g1 = frame(compress_payload(codec, b"".join(b"row-%03d|" % (i % 7) for i in range(37))))
    bad = _bad_blocks(codec)
    assert all(len(b) <= 304 for b in [g0, g1] + [b for _, b in bad])
    runs = [(name, *_run_of([g0, b, g1])) for name, b in bad]
    runs.append(("all", *_run_of([b for _, b in bad])))
    runs.append(("all-reversed", *_run_of([b for _, b in bad][::-1])))
    return runs


def _oracle_status(codec, comp, coff):
    fe = O.decompress_blocks(codec, comp, coff).first_err
    return 0 if fe == NONE else fe & 0xFF


@functools.lru_cache(maxsize=None)
def _oracle_statuses(codec):
    """(the oracle's statuses over every block of the [good, BAD, good] runs, each alone; run name -> the
    status of the run's first error)."""
    runs = _runs(codec)
    seen = set()
    for _, comp, coff in runs[:-2]:
        for k in range(len(coff) - 1):
            a, b = int(coff[k]), int(coff[k + 1])
            seen.add(_oracle_status(codec, comp[a:b], np.array([0, b - a], np.uint64)))
    return seen, {name: _oracle_status(codec, comp, coff) for name, comp, coff in runs}


@pytest.mark.parametrize("codec", CODECS)
@pytest.mark.parametrize("entry", ["run", "once-8", "once-512"])
def test_bad_block_statuses(codec, entry):
    # on the CPU first: the inputs reach every status that applies to the codec (so a weak input cannot hide a
    # path): the two of the frame and the payload's for every codec, a good block beside them, and the length
    # limit where the header declares a length
    want = {0, _abi.SDB_CORRUPT_BLOCK, _abi.SDB_CHECKSUM_MISMATCH, _abi.SDB_DECOMPRESSION_ERROR}
    if codec in LZ:
        want.add(_abi.SDB_LIMIT_EXCEEDED)
    seen, by_name = _oracle_statuses(codec)
    assert seen == want, (seen, want)
    assert by_name["garbage"] == _abi.SDB_DECOMPRESSION_ERROR and by_name["garbage-crc"] == _abi.SDB_CHECKSUM_MISMATCH
    assert by_name["all"] == by_name["empty"] == _abi.SDB_CORRUPT_BLOCK  # the first block of the run
    assert by_name["all-reversed"] != by_name["all"]                    # its last block is of another kind
    for name, comp, coff in _runs(codec):
        if entry == "run":
            err = check_run(codec, comp, coff)[3]
        else:
            err = check_once(codec, comp, coff, int(entry.split("-")[1]))[3]
        # (the helpers assert err == the oracle's first_err, the lengths and the bytes)
        if name not in ("all", "all-reversed"):
            assert err == (NONE if by_name[name] == 0 else (1 << 8) | by_name[name]), name
        else:
            assert err >> 8 == 0, name
