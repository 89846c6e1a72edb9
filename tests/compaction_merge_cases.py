"""The model of a compaction with a merge operator: MergeOperatorIterator as compaction and memtable flush
configure it (merge_operator.rs:324-485 with merge_different_expire_ts = false and snapshot_barrier_seq =
retention_min_seq; compactor_executor.rs:390-400, flush.rs:212-222), restated literally over the entries in
MergeIterator order, in front of the pinned C oracle, which still does retention, cuts and encode.

Entries are (key, kind, value, seq, create_ts, expire_ts) as everywhere in the tests; a run is a list of them,
key ascending and seq descending."""
import json
import os

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd.batch import Run

V, M, T = _abi.KIND_VALUE, _abi.KIND_MERGE, _abi.KIND_TOMBSTONE
MERGE_BATCH_SIZE = 100  # merge_operator.rs:194
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "compaction_merge_cases.json")))["cases"]


class Bracket:
    """An operator whose output shows the call structure (StringConcat is associative and cannot see batching)."""

    @staticmethod
    def merge_batch(key, existing, operands):
        return b"(" + (existing or b"") + b"|" + b",".join(operands) + b")"


def merged_order(runs):
    """MergeIterator order (merge_iterator.rs:55-69): key ascending, seq descending, then run, then position."""
    tagged = [(e[0], -e[3], ri, i, e) for ri, r in enumerate(runs) for i, e in enumerate(r)]
    tagged.sort(key=lambda t: t[:4])
    return [t[4] for t in tagged]


def collapse(runs, barrier, op, stats=None, heads=None):
    """The stream MergeOperatorIterator yields over the runs' merged order.  barrier: snapshot_barrier_seq or None.
    stats (a dict, optional) receives the sdb_merge_op_stats counts; heads (a list, optional) the merged position
    of every chain's first link."""
    s = merged_order(runs)
    st = dict(groups=0, links=0, link_bytes=0, merged_bytes=0, operator_calls=0)
    out, i = [], 0
    while i < len(s):
        key, kind, val, seq, cts, ets = s[i]
        if kind != M:                                  # :474-476
            out.append(s[i])
            i += 1
            continue
        if barrier is not None and seq > barrier:      # :465-469, strict
            out.append(s[i])
            i += 1
            continue
        # merge_with_older_entries (:371-447)
        first_expire_ts = ets
        max_create, min_expire = None, None

        def track(e):                                  # MergeTracker::update (:262-303)
            nonlocal max_create, min_expire
            if e[4] is not None:
                max_create = e[4] if max_create is None else max(max_create, e[4])
            if e[5] is not None:
                min_expire = e[5] if min_expire is None else min(min_expire, e[5])

        results, batch, base, j = [], [], None, i
        if heads is not None:
            heads.append(i)

        def process_batch():
            batch.reverse()
            for e in batch:
                track(e)
            st["operator_calls"] += 1
            results.append(op.merge_batch(key, None, [e[2] for e in batch]))
            batch.clear()

        while j < len(s):
            e = s[j]
            if e[0] != key or e[5] != first_expire_ts:  # is_matching_entry (:330-335): not consumed
                break
            st["links"] += 1
            st["link_bytes"] += len(e[2]) if e[1] != T else 0
            j += 1
            if e[1] != M:                              # a value or a tombstone: the base, consumed
                base = e
                break
            batch.append(e)
            if len(batch) >= MERGE_BATCH_SIZE:
                process_batch()
        if batch:
            process_batch()
        base_value = base[2] if base is not None and base[1] == V else None
        if base is not None:
            track(base)
        results.reverse()
        st["operator_calls"] += 1
        final = op.merge_batch(key, base_value, results)
        st["groups"] += 1
        st["merged_bytes"] += len(final)
        out.append((key, V if base is not None else M, final, seq, max_create, min_expire))
        i = j
    if stats is not None:
        stats.update(st)
    return out


def barrier_of(ret):
    return int(ret.min_seq) if ret.has_min_seq else None


def expected(runs, ret, prm, max_sst_size, op, stats=None):
    """What the job must give: O.compact over the collapsed stream as one run, operands passed on.
    Returns (merged Batch, MergeSummary, cuts, [SstResult])."""
    r = _abi.Retention.from_buffer_copy(ret)
    r.merge_operands = 1
    col = collapse(runs, barrier_of(ret), op, stats)
    merged, sm, cuts, ssts = O.compact([Run.from_entries(col)], r, prm, max_sst_size)
    return merged, sm, cuts, ssts


def fixture_entries(rows):
    """A fixture case's rows, (key, kind, value, seq, expire_ts), as one sorted run of entries."""
    es = [(k.encode(), kind, v.encode() if kind != T else b"", seq, None, x) for k, kind, v, seq, x in rows]
    return es


def fixture_run(case):
    return sorted(fixture_entries(case["entries"]), key=lambda e: (e[0], -e[3]))
