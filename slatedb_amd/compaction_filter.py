"""Compaction filters for the device compactor (sdb_compactor_run_filtered / _run_ssts_filtered): the decision
constants, the job context a CompactionFilterSupplier receives, and the two forms a filter takes here.

The C callback sees the retained stream in batches (include/slatedb_amd.h, "Compaction filters and resumed jobs").
  BatchFilter   the direct form for numpy users: filter_batch(rows) over a Rows view of one call;
  PerEntry      the reference's trait, filter(entry) -> KEEP | DROP | TOMBSTONE | (VALUE, b) | (MERGE, b) and
                on_compaction_end(), wrapped into the batch form.
callbacks(flt) turns either into the sdb_compaction_filter struct.  An exception in a filter never unwinds through
the C frames: it becomes a non-zero return (the job fails with SDB_COMPACTION_FILTER_ERROR) and is kept in the
returned state's "error"."""
import collections
import ctypes as C

import numpy as np

from . import _abi

KEEP, DROP, TOMBSTONE, VALUE, MERGE = _abi.CF_KEEP, _abi.CF_DROP, _abi.CF_TOMBSTONE, _abi.CF_VALUE, _abi.CF_MERGE

Entry = collections.namedtuple("Entry", "key kind value seq create_ts expire_ts")  # value: None when not gathered


class CompactionJobContext(collections.namedtuple(
        "CompactionJobContext", "destination is_dest_last_run compaction_clock_tick retention_min_seq")):
    """What create_compaction_filter receives (compaction_filter.rs:81-95)."""

    @classmethod
    def from_retention(cls, ret, destination=0):
        return cls(destination, bool(ret.filter_tombstone), int(ret.compaction_start_ts),
                   int(ret.min_seq) if ret.has_min_seq else None)


def _view(ptr, count, dtype):
    if not ptr or not count:
        return np.zeros(0, dtype)
    nbytes = count * np.dtype(dtype).itemsize
    return np.frombuffer((C.c_uint8 * nbytes).from_address(ptr), dtype=dtype, count=count)


class Rows:
    """One filter call: rows [first, first + n) of the retained stream as numpy views of the pinned host arrays
    (valid during the call only).  key_off / val_off are absolute offsets into key_bytes / val_bytes; val_bytes is
    None unless the filter asked for values."""

    def __init__(self, kb, first):
        n = self.n = int(kb.n)
        self.first = int(first)
        self.key_off = _view(kb.key_off, n + 1, np.uint64)
        self.val_off = _view(kb.val_off, n + 1, np.uint64)
        self.kind = _view(kb.kind, n, np.uint8)
        self.seq = _view(kb.seq, n, np.uint64)
        self.create_ts = _view(kb.create_ts, n, np.int64)
        self.expire_ts = _view(kb.expire_ts, n, np.int64)
        self.ts_mask = _view(kb.ts_mask, n, np.uint8)
        self.key_bytes = _view(kb.key_bytes, int(self.key_off[n]) if n else 0, np.uint8)
        self.val_bytes = _view(kb.val_bytes, int(self.val_off[n]) if n else 0, np.uint8) if kb.val_bytes else None

    def key(self, i):
        return self.key_bytes[int(self.key_off[i]):int(self.key_off[i + 1])].tobytes()

    def value(self, i):
        if self.val_bytes is None:
            return None
        return self.val_bytes[int(self.val_off[i]):int(self.val_off[i + 1])].tobytes()

    def entry(self, i):
        m = int(self.ts_mask[i])
        return Entry(self.key(i), int(self.kind[i]), self.value(i), int(self.seq[i]),
                     int(self.create_ts[i]) if m & _abi.TS_CREATE else None,
                     int(self.expire_ts[i]) if m & _abi.TS_EXPIRE else None)


class BatchFilter:
    """The batch form.  filter_batch(rows) returns None (keep every row), an array of n decisions, or, with VALUE /
    MERGE rows, (decisions, replacements): either {row index within the call: replacement bytes}, or the packed form
    (arena, offsets): the replacements of the call's VALUE / MERGE rows in row order, replacement j =
    arena[offsets[j]:offsets[j + 1]] (a uint8 array or bytes, and m + 1 offsets), which costs no Python object per
    row."""
    want_values = False
    batch_rows = 0  # rows per call; 0: the whole stream in one call

    def filter_batch(self, rows):
        return None

    def on_compaction_end(self):
        pass


class PerEntry(BatchFilter):
    """A per-entry filter (an object with filter(entry) and, optionally, on_compaction_end()) as a BatchFilter."""

    def __init__(self, inner, batch_rows=0, want_values=True):
        self.inner, self.batch_rows, self.want_values = inner, batch_rows, want_values

    def filter_batch(self, rows):
        dec, vals = np.zeros(rows.n, np.uint8), {}
        for i in range(rows.n):
            r = self.inner.filter(rows.entry(i))
            if isinstance(r, tuple):
                dec[i], vals[i] = r
            else:
                dec[i] = r
        return dec, vals

    def on_compaction_end(self):
        end = getattr(self.inner, "on_compaction_end", None)
        if end is not None:
            end()


class PrefixTombstoneFilter:
    """The reference's documentation example: every entry whose key starts with `prefix` becomes a tombstone."""

    def __init__(self, prefix):
        self.prefix, self.tombstone_count, self.ended = bytes(prefix), 0, 0

    def filter(self, entry):
        if entry.key.startswith(self.prefix):
            self.tombstone_count += 1
            return TOMBSTONE
        return KEEP

    def on_compaction_end(self):
        self.ended += 1


def callbacks(flt, batch_rows=None, want_values=None):
    """`flt` (a BatchFilter, or an object with filter(entry): wrapped in PerEntry) -> (sdb_compaction_filter, state).
    The caller keeps both alive for the job.  state["error"]: the exception that failed the job, if any.  An
    sdb_compaction_filter the caller built itself passes through as it is."""
    if isinstance(flt, _abi.CompactionFilter):
        return flt, {"error": None, "bufs": None, "filter": None}
    if not hasattr(flt, "filter_batch"):
        flt = PerEntry(flt)
    state = {"error": None, "bufs": None, "filter": flt}

    def call(ctx, rows_p, first, decision, new_val, new_len):
        try:
            rows = Rows(rows_p.contents, first)
            res = flt.filter_batch(rows)
            if res is None:
                return 0
            dec, vals = res if isinstance(res, tuple) else (res, {})
            d = np.ascontiguousarray(dec, np.uint8)
            if d.shape != (rows.n,):
                raise ValueError("filter_batch returned %r decisions for %d rows" % (d.shape, rows.n))
            if rows.n:
                C.memmove(decision, d.ctypes.data, rows.n)
            if not isinstance(vals, dict):  # the packed form: no Python object per replacement
                arena, off = vals
                arena = np.ascontiguousarray(np.frombuffer(arena, np.uint8) if isinstance(arena, (bytes, bytearray))
                                             else arena, np.uint8)
                off = np.ascontiguousarray(off, np.uint64)
                idx = np.nonzero((d == VALUE) | (d == MERGE))[0]
                if len(off) != len(idx) + 1 or off[-1] > arena.size or np.any(off[1:] < off[:-1]):
                    raise ValueError("%d offsets over %d bytes for %d replaced rows" % (len(off), arena.size, len(idx)))
                if len(idx):
                    nv = _view(C.addressof(new_val.contents), rows.n, np.uint64)
                    nl = _view(C.addressof(new_len.contents), rows.n, np.uint64)
                    nv[idx] = np.uint64(arena.ctypes.data) + off[:-1]
                    nl[idx] = off[1:] - off[:-1]
                state["bufs"] = arena  # alive until the next call
                return 0
            bufs = []
            for i, b in vals.items():
                if not 0 <= i < rows.n:
                    raise IndexError(i)
                b = bytes(b)
                buf = C.create_string_buffer(b, max(len(b), 1))
                bufs.append(buf)
                new_val[i] = C.addressof(buf)
                new_len[i] = len(b)
            state["bufs"] = bufs  # alive until the next call: the library copies them before it
            return 0
        except Exception as e:  # never unwind through the C frames
            state["error"] = e
            return 1

    def end(ctx):
        try:
            flt.on_compaction_end()
            return 0
        except Exception as e:
            state["error"] = e
            return 1

    cf = _abi.CompactionFilter(_abi.COMPACTION_FILTER_FN(call), _abi.COMPACTION_END_FN(end), None,
                               flt.batch_rows if batch_rows is None else batch_rows,
                               int(bool(flt.want_values if want_values is None else want_values)), 0)
    return cf, state


def cursor(key, seq):
    """(sdb_resume_cursor, the buffer it points into) of the last row an interrupted job wrote."""
    key = bytes(key)
    buf = C.create_string_buffer(key, max(len(key), 1))
    return _abi.ResumeCursor(C.addressof(buf), len(key), int(seq)), buf
