"""The host half of the WAL replay (include/slatedb_amd.h, "WAL replay / device memtable") and its model.

  estimate_encoded_size_compacted   SsTableFormat::estimate_encoded_size_compacted (format/sst.rs:1041-1160)
  split_tables                      the W6 walk of WalReplayIterator::next (wal_replay.rs:119-184) over the
                                    per-batch facts sdb_wal_replay_sort returns
  replay_model                      W1-W7 in plain Python (a dict keyed by (key, seq) per table, `sorted`):
                                    the oracle of the tests

Rows are the tuples Batch.from_entries takes: (key, kind, value, seq, create_ts | None, expire_ts | None);
a batch is the list of rows of one WalRows in insertion order.
"""
from . import _abi

I64_MIN = -(1 << 63)
U64_MAX = (1 << 64) - 1

# format/sst.rs:143-150
SIZEOF_U8, SIZEOF_U16, SIZEOF_U32, SIZEOF_U64 = 1, 2, 4, 8
CHECKSUM_SIZE = SIZEOF_U32
OFFSET_SIZE = SIZEOF_U16
METADATA_OFFSET_SIZE = SIZEOF_U64
VERSION_SIZE = SIZEOF_U16


def row_estimated_size(row):
    """RowEntry::estimated_size (types.rs:48-60); a tombstone's value length is 0."""
    key, kind, value, _seq, cts, ets = row
    vlen = 0 if kind == _abi.KIND_TOMBSTONE else len(value or b"")
    return len(key) + vlen + 8 + (8 if cts is not None else 0) + (8 if ets is not None else 0)


def _filter_name_len(prm):
    from .runtime import filter_name
    return len(filter_name(prm))


def estimate_encoded_size_compacted(prm, entry_num, size):
    """format/sst.rs:1041-1064 for the format `prm` (an sdb_sst_params: block_size, bloom_bits_per_key,
    min_filter_keys and the filter policy's name; no bits per key = no filter policy)."""
    if entry_num == 0:
        return 0
    first_key = 12  # guess_at_average_first_key_size_bytes
    # SstRowCodecV0::estimate_encoded_size (format/row.rs:149-157): prefix len u16, suffix len u16, value len u32, flags u8
    encoded = size + (2 + 2 + 4 + 1) * entry_num
    blocks = -(-encoded // prm.block_size)
    # Block::estimate_encoded_size (format/block.rs:64-73)
    ans = encoded + OFFSET_SIZE * entry_num + CHECKSUM_SIZE * blocks
    # the index (format/sst.rs:1107-1110)
    ans += blocks * (first_key + OFFSET_SIZE) + CHECKSUM_SIZE
    # SsTableInfo (:1112-1129): first entry, index / filter / stats offset + length, compression format, sst type,
    # last entry, filter format, checksum
    ans += first_key + 2 * SIZEOF_U64 + 2 * SIZEOF_U64 + SIZEOF_U8 + SIZEOF_U8 + first_key + 2 * SIZEOF_U64 + SIZEOF_U8 + CHECKSUM_SIZE
    ans += METADATA_OFFSET_SIZE + VERSION_SIZE
    # the filter (:1136-1152): composite framing u16, per filter u16 + name + u64 + BloomFilter::estimate_encoded_size
    # (filter.rs:114-118: u32 arithmetic, + the probe count u16), one checksum
    if prm.bloom_bits_per_key and entry_num >= prm.min_filter_keys:
        bits = (entry_num * prm.bloom_bits_per_key) & 0xFFFFFFFF
        ans += 2 + (2 + _filter_name_len(prm) + 8) + (-(-bits // 8) + 2) + CHECKSUM_SIZE
    # the stats (:1154-1160)
    ans += 3 * SIZEOF_U64 + 2 * SIZEOF_U64 + blocks * 3 * SIZEOF_U16 + CHECKSUM_SIZE
    return ans


def split_tables(facts, prm, max_memtable_bytes):
    """W6: batch indices [0, ..., nbatches] of the tables' first batches.  facts: per batch an object (or dict)
    with .rows and .bytes.  No batches: no table."""
    get = (lambda f, k: f[k]) if facts and isinstance(facts[0], dict) else getattr
    cuts, rows, size = [0], 0, 0
    for b, f in enumerate(facts):
        rows += get(f, "rows")
        size += get(f, "bytes")
        if rows and estimate_encoded_size_compacted(prm, rows, size) >= max_memtable_bytes and b + 1 < len(facts):
            cuts.append(b + 1)
            rows = size = 0
    if facts:
        cuts.append(len(facts))
    return cuts


def table_metadata(facts, cuts, last_l0_seq=0, last_l0_clock_tick=I64_MIN, wal_ids=None):
    """W7 for the tables split_tables cut: per table a dict with the KVTableMetadata words, the replay's running
    last_seq / last_tick (ReplayedMemtable) and last_wal_id (wal_ids: last_consumed_wal_file_id per batch)."""
    get = (lambda f, k: f[k]) if facts and isinstance(facts[0], dict) else getattr
    out, run_seq, run_tick = [], last_l0_seq, last_l0_clock_tick
    for t in range(len(cuts) - 1):
        m = {"batches": (cuts[t], cuts[t + 1]), "entry_num": 0, "entries_size_in_bytes": 0, "first_seq": U64_MAX,
             "last_seq": 0, "last_tick": I64_MIN}
        for b in range(cuts[t], cuts[t + 1]):
            f = facts[b]
            m["entry_num"] += get(f, "rows")
            m["entries_size_in_bytes"] += get(f, "bytes")
            if get(f, "rows"):
                m["first_seq"] = min(m["first_seq"], get(f, "min_seq"))
                m["last_seq"] = max(m["last_seq"], get(f, "max_seq"))
            if get(f, "any_create_ts"):
                m["last_tick"] = max(m["last_tick"], get(f, "max_create_ts"))
        run_seq = max(run_seq, m["last_seq"])
        run_tick = max(run_tick, m["last_tick"])
        m["replay_last_seq"], m["replay_last_tick"] = run_seq, run_tick
        m["last_wal_id"] = None if wal_ids is None else wal_ids[cuts[t + 1] - 1]
        out.append(m)
    return out


def order_violation(batches):
    """W2: the first batch whose smallest seq does not exceed the largest seq of every earlier batch, or None."""
    top = None
    for b, rows in enumerate(batches):
        if not rows:
            continue
        seqs = [r[3] for r in rows]
        if top is not None and min(seqs) <= top:
            return b
        top = max(seqs) if top is None else max(top, max(seqs))
    return None


def replay_model(batches, min_seq, prm, max_memtable_bytes, last_l0_seq=0, last_l0_clock_tick=I64_MIN, wal_ids=None):
    """W1-W7.  min_seq None: no filter.  Returns a dict: status, first_error_entry, facts (a dict per batch),
    summary, cuts, tables (the W7 dicts, each with "rows": its rows in table order)."""
    n = sum(len(b) for b in batches)
    bad = order_violation(batches)
    if bad is not None:
        return {"status": _abi.SDB_INVALID_ARGUMENT, "first_error_entry": bad, "facts": None, "cuts": None, "tables": [],
                "summary": {"rows_in": n, "rows_skipped": 0, "rows_replaced": 0, "rows_out": 0, "key_bytes": 0,
                            "val_bytes": 0}}
    facts, kept = [], []
    for rows in batches:
        table = {}  # by W2 an equal (key, seq) pair lies in one batch
        f = {"rows": 0, "bytes": 0, "replaced": 0, "min_seq": 0, "max_seq": 0, "max_create_ts": 0, "any_create_ts": 0}
        passed = [r for r in rows if min_seq is None or r[3] > min_seq]  # W1
        for r in passed:
            table[(r[0], r[3])] = r  # W4: the later arrival replaces
        if passed:
            f["min_seq"], f["max_seq"] = min(r[3] for r in passed), max(r[3] for r in passed)
            ticks = [r[4] for r in passed if r[4] is not None]
            if ticks:
                f["any_create_ts"], f["max_create_ts"] = 1, max(ticks)
        f["rows"] = len(table)
        f["replaced"] = len(passed) - len(table)
        f["bytes"] = sum(row_estimated_size(r) for r in table.values())
        facts.append(f)
        kept.append(list(table.values()))
    cuts = split_tables(facts, prm, max_memtable_bytes)
    tables = table_metadata(facts, cuts, last_l0_seq, last_l0_clock_tick, wal_ids)
    for t, m in enumerate(tables):
        rows = [r for b in range(cuts[t], cuts[t + 1]) for r in kept[b]]
        m["rows"] = sorted(rows, key=lambda r: (r[0], -r[3]))  # W3
    out_rows = [r for m in tables for r in m["rows"]]
    summary = {"rows_in": n, "rows_skipped": n - sum(f["rows"] + f["replaced"] for f in facts),
               "rows_replaced": sum(f["replaced"] for f in facts), "rows_out": len(out_rows),
               "key_bytes": sum(len(r[0]) for r in out_rows),
               "val_bytes": sum(0 if r[1] == _abi.KIND_TOMBSTONE else len(r[2] or b"") for r in out_rows)}
    return {"status": _abi.SDB_OK, "first_error_entry": U64_MAX, "facts": facts, "summary": summary, "cuts": cuts,
            "tables": tables}
