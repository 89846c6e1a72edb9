"""Blocks malformed inside a valid CRC, on the CPU: the catalogue of tests/malformed_blocks.py proves itself
against the literal walker, the walker and the oracle agree on every case, lookups that end before a faulty
row are unharmed, and the oracle does not read past the bytes it judges (a sanitized stand-alone program).

Where the expectations come from: every status is the walker's, which restates the reference's text, and the
oracle must return the same -- except the descending cases marked desc_from == "header": there the walker
states the descending rule of include/slatedb_amd.h (a restart table that descending iteration cannot
follow is SDB_CORRUPT_BLOCK), which the oracle does not return (test_descending_irregular_oracle_runs), so
only the neighbours of such a block are compared with the oracle."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

from . import malformed_blocks as MB
from .scan_cases import row_tuples

SHAPE_NAMES = list(MB.SHAPES)


def block_rows(dec, k, descending):
    """The rows of block k of an oracle (or device) decode, in iteration order."""
    bes = np.asarray(dec.block_entry_start).astype(np.int64)
    rows = row_tuples(dec)
    n = len(rows)
    return rows[n - bes[k + 1]:n - bes[k]] if descending else rows[bes[k]:bes[k + 1]]


def walker_rows(payload, version, descending, start):
    st, rows = MB.walk(payload, version, descending)
    return st, [(k, vo + start if vl else 0, vl, sq, f, c, e) for (k, vo, vl, sq, f, c, e) in rows]


def check_against_walker(dec, payloads, block_off, version, descending, what, own_status=True):
    """Status, bad_block and every surviving row of a decode of `payloads` against the walker.
    own_status False: the failing blocks' own statuses are not compared (the header's rule)."""
    want = [walker_rows(p, version, descending, int(block_off[k])) for k, p in enumerate(payloads)]
    bad = [k for k, (st, _) in enumerate(want) if st]
    if own_status:
        assert dec.status == (want[bad[0]][0] if bad else 0), what
        assert sorted(dec.bad_block.tolist()) == bad, what
    for k, (st, rows) in enumerate(want):
        if own_status or not st:
            assert block_rows(dec, k, descending) == rows, (what, k)


@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_catalogue_proves_itself(name):
    S = MB.shape(name)
    for desc in (False, True):
        assert MB.walk(S.layout.payload, S.version, desc)[0] == 0
    singles, doubles = MB.singles(name), MB.doubles(name)
    assert len({v.id for v in singles + doubles}) == len(singles) + len(doubles)
    for v in singles:
        for desc in (False, True):
            assert MB.walk(v.payload, S.version, desc)[0] == v.status(desc), (v.id, desc)
    for v in doubles:
        for desc in (False, True):
            alone = [MB.walk(p, S.version, desc)[0] for p in v.parts]
            assert sorted(alone) == [MB.FLAGS, MB.CORRUPT], (v.id, desc, alone)
            assert MB.walk(v.payload, S.version, desc)[0] in alone, (v.id, desc)


def test_catalogue_covers_both_statuses_and_orders():
    """The double faults tell ascending from descending: some variant reports another status each way (a block
    of one restart region is decoded in one direction either way)."""
    for name in SHAPE_NAMES:
        S = MB.shape(name)
        if S.version == 2 and S.layout.count == 1:
            continue
        differ = [v.id for v in MB.doubles(name)
                  if MB.walk(v.payload, S.version, False)[0] != MB.walk(v.payload, S.version, True)[0]]
        assert differ, name


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_walker_and_oracle_agree(name, desc):
    S = MB.shape(name)
    good0, good2 = S.payloads[0], S.payloads[2]
    for i, v in enumerate(MB.variants(name)):
        payloads = [good0, v.payload, good2]
        data, off = MB.arena(payloads, MB.lead_for(payloads, 1, (0, 1, 15)[i % 3]))
        dec = O.decode_blocks(data, off, S.version, descending=desc)
        header = desc and v.desc_from == "header"
        check_against_walker(dec, payloads, off, S.version, desc, (name, v.id), own_status=not header)
        if header:
            assert MB.walk(v.payload, S.version, True)[0] == MB.CORRUPT


@pytest.mark.parametrize("version", [1, 2])
def test_tiny_blocks(version):
    S = MB.shape("v2-spec-4regions-1k" if version == 2 else "v1-small-1k")
    for name, payload, want in MB.TINY:
        for desc in (False, True):
            assert MB.walk(payload, version, desc)[0] == want[version][desc], (name, desc)
            payloads = [S.payloads[0], payload, S.payloads[2]]
            data, off = MB.arena(payloads)
            dec = O.decode_blocks(data, off, version, descending=desc)
            check_against_walker(dec, payloads, off, version, desc, (name, version, desc))


# faults a key-only decode does not see (a seek's binary search may probe any row's key)
LOOKUP_FAULTS = ("flags-10@", "vl-ends-1-past-end-9@", "shared-over-prev@", "v1-flags-10@", "v1-value-1-past-end@")


def lookup_cases(name):
    """(variant, [key before the faulty row, its key, the key after it]) for the faults of LOOKUP_FAULTS."""
    S = MB.shape(name)
    out = [(v, MB.lookup_keys(S, v)) for v in MB.singles(name)
           if v.id.startswith(LOOKUP_FAULTS) and v.row]
    assert out, name
    return out


FIELDS = [f for f, _ in O.LOOKUP_FIELDS]


def lookup(S, data, off, keys, desc):
    return O.sst_lookup(data, off, S.index_keys, S.index_key_off, keys, descending=desc, sst_version=S.version)


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("name", SHAPE_NAMES)
def test_lookup_before_the_fault_is_unharmed(name, desc):
    """A seek that ends before the faulty row returns what the clean SST returns; a seek that reaches it reports
    the row's status.  (Ascending the seek walks up to the key; descending it loads whole restart regions, so
    "before" is a row of an earlier region where the block has more than one.)"""
    S = MB.shape(name)
    cdata, coff = S.sst_with(S.layout.payload)
    for v, qs in lookup_cases(name):
        data, off = S.sst_with(v.payload)
        assert np.array_equal(off, coff)  # the lookup faults are in place
        keys = qs
        got, clean = lookup(S, data, off, keys, desc), lookup(S, cdata, coff, keys, desc)
        assert clean.status.tolist() == [0, 0, 0]
        if desc and (S.version == 2 and S.layout.rows[v.row]["region"] == 0):
            # no earlier region: "before" is the row just before the faulty one, and the region is loaded whole
            assert got.status[0] == v.status(desc), v.id
        else:
            for f in FIELDS:
                assert getattr(got, f)[0] == getattr(clean, f)[0], (v.id, f)
        assert got.status[1] == v.status(desc), v.id
        # past the fault: ascending the seek has to walk over the faulty row when it is in the same region
        # or the block's restart search lands there; the status is the row's or none, never another
        assert got.status[2] in (0, v.status(desc)), v.id


# --- the oracle under the address and undefined-behaviour sanitizers ---------------------------------------
def write_catalogue(path):
    """Every variant of every shape as [good, mutated, good] with exact-length data (no tail pad), the walker's
    statuses and the lookup keys, for oracle/malformed_check.c."""
    cases = []
    for name in SHAPE_NAMES:
        S = MB.shape(name)
        for v in MB.variants(name):
            payloads = [S.payloads[0], v.payload, S.payloads[2]]
            header = v.desc_from == "header"
            cases.append((S, payloads, MB.walk(v.payload, S.version)[0],
                          -1 if header else MB.walk(v.payload, S.version, True)[0], MB.lookup_keys(S, v)))
    for version in (1, 2):
        S = MB.shape("v2-spec-4regions-1k" if version == 2 else "v1-small-1k")
        for _, payload, want in MB.TINY:
            cases.append((S, [S.payloads[0], payload, S.payloads[2]], want[version][0], want[version][1], []))
    with open(path, "wb") as f:
        f.write(b"MBC1" + struct.pack("<I", len(cases)))
        for S, payloads, asc, desc, keys in cases:
            data, off = MB.arena(payloads)
            data = data[:len(data) - MB.TAIL_PAD].tobytes()
            ik = S.index_keys.tobytes()
            iko = np.asarray(S.index_key_off[:4], np.uint64)
            f.write(struct.pack("<IIiiIQQ", S.version, 3, asc, desc, len(keys), len(data), int(iko[3])))
            f.write(np.asarray(off, "<u8").tobytes() + iko.astype("<u8").tobytes())
            f.write(data + ik[:int(iko[3])])
            for k in keys:
                f.write(struct.pack("<I", len(k)) + k)
    return len(cases)


def test_oracle_reads_no_byte_past_the_block(tmp_path):
    if shutil.which(os.environ.get("CC", "gcc")) is None:
        pytest.fail("no C compiler for the sanitized oracle program")
    here = os.path.dirname(os.path.abspath(O.__file__))
    exe = str(tmp_path / "malformed_check")
    subprocess.check_call(["make", "-s", "-C", here, "malformed_check", "MALFORMED_CHECK=" + exe])
    cat = str(tmp_path / "catalogue.bin")
    n = write_catalogue(cat)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([exe, cat], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert ("%d cases ok" % n) in r.stdout
