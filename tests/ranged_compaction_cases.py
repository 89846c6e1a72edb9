"""Expected results of sdb_compactor_run_ssts_ranged: rules R1-R3 and R6 of include/slatedb_amd.h restated on the
host, in front of the pinned C oracle, which still does merge, retention, cuts and encode.
  R1  V[i] = job range intersected with visible[i] (projected_read_cases.intersect), None when empty;
  R2  the blocks input i reads: scan_cases.partitions_covering_range over its index keys (O.sst_index_keys);
  R3  its rows: those whose key V[i] contains (scan_cases.contains); a run is its inputs' rows in input order.
A range is (start, start_kind, end, end_kind), None meaning unbounded / the whole SST."""
import types

import numpy as np

from oracle import oracle as O
from slatedb_amd import _abi
from slatedb_amd.batch import Batch, Run

from .projected_read_cases import OPEN, intersect
from .scan_cases import contains, partitions_covering_range

V, M, T = _abi.KIND_VALUE, _abi.KIND_MERGE, _abi.KIND_TOMBSTONE


def batch_of_run(r):
    kind = np.where(r.flags & _abi.FLAG_TOMBSTONE, T, np.where(r.flags & _abi.FLAG_MERGE_OPERAND, M, V)).astype(np.uint8)
    mask = (np.where(r.flags & _abi.FLAG_HAS_EXPIRE_TS, _abi.TS_EXPIRE, 0) |
            np.where(r.flags & _abi.FLAG_HAS_CREATE_TS, _abi.TS_CREATE, 0)).astype(np.uint8)
    end = r.val_off[-1] + r.val_len[-1] if r.n else 0
    return Batch(r.key_arena, r.key_off, r.val_base, np.concatenate([r.val_off, [end]]).astype(np.uint64), kind, r.seq,
                 r.create_ts, r.expire_ts, mask)


def run_keys(r):
    ko, ka = r.key_off.astype(np.int64).tolist(), r.key_arena.tobytes()
    return [ka[ko[i]:ko[i + 1]] for i in range(r.n)]


def build_job(runs, prm_kw, splits=None):
    """Each run encoded by the oracle as splits[r] consecutive SSTs -> a job: .inputs (host arrays of each SST: data,
    block_off, index_keys / index_key_off, the SstStats counts; .ikeys its index keys, .first_row each block's first
    row, .ref its rows as the reference reads them back, .keys their keys), .run_start, .version."""
    version = prm_kw.get("sst_version", 2)
    inputs, run_start = [], [0]
    for ri, r in enumerate(runs):
        b, split = batch_of_run(r), (splits[ri] if splits else 1)
        cuts = np.linspace(0, b.n, split + 1).astype(int)
        for i in range(split):
            part = b.slice(cuts[i], cuts[i + 1])
            enc = O.encode_sst(part, O.params(**prm_kw))
            sm = enc.summary
            assert sm.status == 0
            bo = enc.block_off.astype(np.uint64)
            nb = len(bo) - 1
            blocks = enc.data[:int(bo[-1])]
            d = O.decode_blocks(blocks, bo, version)
            assert d.status == 0 and d.n == part.n
            ref = Run(d.key_arena, d.key_off, blocks, d.val_off, d.val_len, d.seq, d.flags, d.create_ts, d.expire_ts)
            ikb, iko = O.sst_index_keys(part, enc)
            o = iko.astype(np.int64).tolist()
            inputs.append(types.SimpleNamespace(
                data=np.concatenate([enc.data, np.zeros(16, np.uint8)]), block_off=bo,
                index_keys=np.concatenate([ikb, np.zeros(1, np.uint8)]), index_key_off=iko,
                num_entries=int(sm.num_entries), key_bytes=int(sm.raw_key_size), val_bytes=int(sm.raw_val_size),
                ikeys=[ikb.tobytes()[o[k]:o[k + 1]] for k in range(nb)],
                first_row=np.concatenate([np.asarray(enc.block_first_entry[:nb], np.int64), [part.n]]),
                ref=ref, keys=run_keys(ref)))
        run_start.append(len(inputs))
    return types.SimpleNamespace(inputs=inputs, run_start=run_start, version=version)


MAX_SST = 32 << 10  # of the small job's outputs: several SSTs for the whole job
_JOBS = {}


def small_job(seed=41, version=2, block_size=256):
    """The shape every ranged test shares: three L0 runs and one sorted run of three SSTs over about 2,000 keys of up to
    four versions, in blocks of `block_size` bytes (some tens of blocks per input).  Built once per argument set;
    read-only."""
    from .test_gpu_compaction import big_runs
    key = (seed, version, block_size)
    if key not in _JOBS:
        runs = big_runs(seed, 2000, 4, maxver=4, vmax=40)
        _JOBS[key] = build_job(runs, dict(block_size=block_size, sst_version=version), splits=[1, 1, 1, 3])
        assert all(len(x.ikeys) >= 8 for x in _JOBS[key].inputs)
    return _JOBS[key]


def metas(job):
    """The planner's view of the job's inputs (slatedb_amd.subcompaction.SstMeta)."""
    from slatedb_amd.subcompaction import SstMeta
    return [SstMeta(x.ikeys, x.block_off[:-1], int(x.block_off[-1])) for x in job.inputs]


def upload(job):
    """The job's inputs as Compactor.run_ssts_ranged takes them (device tensors)."""
    import torch
    dev = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()  # noqa: E731
    return [types.SimpleNamespace(data=dev(x.data.copy()), block_off=dev(x.block_off), index_keys=dev(x.index_keys),
                                  index_key_off=dev(x.index_key_off), num_entries=x.num_entries, key_bytes=x.key_bytes,
                                  val_bytes=x.val_bytes) for x in job.inputs]


def view(job_range, vis):
    """R1: V of an input, or None when it is empty."""
    return intersect(job_range or OPEN, vis or OPEN)


def take_rows(r, idx):
    idx = np.asarray(idx, np.int64)
    ko = r.key_off.astype(np.int64)
    lens = (ko[1:] - ko[:-1])[idx]
    arena = np.concatenate([r.key_arena[ko[i]:ko[i + 1]] for i in idx]) if len(idx) else np.zeros(0, np.uint8)
    return Run(arena, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64), r.val_base, r.val_off[idx], r.val_len[idx],
               r.seq[idx], r.flags[idx], r.create_ts[idx], r.expire_ts[idx])


def concat_runs(parts):
    if not parts:
        z = np.zeros(0, np.int64)
        return Run(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8), z, z, z, z, z, z)
    kbase = np.cumsum([0] + [len(p.key_arena) for p in parts])
    vbase = np.cumsum([0] + [len(p.val_base) for p in parts])
    cat = lambda f: np.concatenate([getattr(p, f) for p in parts])  # noqa: E731
    koff = np.concatenate([p.key_off[:-1] + np.uint64(kbase[i]) for i, p in enumerate(parts)] + [[np.uint64(kbase[-1])]])
    voff = np.concatenate([p.val_off + np.uint64(vbase[i]) for i, p in enumerate(parts)])
    return Run(cat("key_arena"), koff.astype(np.uint64), cat("val_base"), voff.astype(np.uint64), cat("val_len"), cat("seq"),
               cat("flags"), cat("create_ts"), cat("expire_ts"))


def clipped(job, job_range=None, projections=None):
    """R1-R3 -> (the job's runs as the ranged job reads them, the sdb_range_job_stats words)."""
    st = dict(inputs_read=0, blocks_total=0, blocks_checked=0, entries_decoded=0, entries_in=0)
    runs = []
    for r in range(len(job.run_start) - 1):
        parts = []
        for i in range(job.run_start[r], job.run_start[r + 1]):
            x = job.inputs[i]
            st["blocks_total"] += len(x.ikeys)
            Vi = view(job_range, projections[i] if projections else None)
            if Vi is None:
                continue
            bs, be = partitions_covering_range(x.ikeys, *Vi)
            if be > bs:
                st["inputs_read"] += 1
                st["blocks_checked"] += be - bs
                st["entries_decoded"] += int(x.first_row[be] - x.first_row[bs])
            rows = [j for j, k in enumerate(x.keys) if contains(k, *Vi)]
            assert all(x.first_row[bs] <= j < x.first_row[be] for j in rows)  # R2 covers R3
            st["entries_in"] += len(rows)
            parts.append(take_rows(x.ref, rows))
        runs.append(concat_runs(parts))
    return runs, st


def covering(job, job_range=None, projections=None):
    """R2: the covering block range of every input (None: V is empty)."""
    out = []
    for i, x in enumerate(job.inputs):
        Vi = view(job_range, projections[i] if projections else None)
        out.append(None if Vi is None else partitions_covering_range(x.ikeys, *Vi))
    return out


def run_entries(r):
    """A Run's rows as the entries (key, kind, value, seq, create_ts, expire_ts) the operator model takes."""
    out, keys = [], run_keys(r)
    for i in range(r.n):
        f = int(r.flags[i])
        kind = T if f & _abi.FLAG_TOMBSTONE else (M if f & _abi.FLAG_MERGE_OPERAND else V)
        vo, vl = int(r.val_off[i]), int(r.val_len[i])
        out.append((keys[i], kind, r.val_base[vo:vo + vl].tobytes() if kind != T else b"", int(r.seq[i]),
                    int(r.create_ts[i]) if f & _abi.FLAG_HAS_CREATE_TS else None,
                    int(r.expire_ts[i]) if f & _abi.FLAG_HAS_EXPIRE_TS else None))
    return out


def expected(job, ret, prm, max_sst_size, job_range=None, projections=None, op=None, mstats=None):
    """What the ranged job must give -> ((merged Batch, MergeSummary, cuts, [SstResult]), range stats)."""
    runs, st = clipped(job, job_range, projections)
    if op is None:
        return O.compact(runs, ret, prm, max_sst_size), st
    from . import compaction_merge_cases as CM
    return CM.expected([run_entries(r) for r in runs], ret, prm, max_sst_size, op, mstats), st
