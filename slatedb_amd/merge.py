"""The host half of a merging read: the user's merge operator over chains the device located.

sdb_lsm_get_merge / sdb_lsm_scan_merge return, per query or row, the links of its operand chain, newest first:
merge operands, then at most one base value.  fold() calls the operator on them exactly as
MergeOperatorIterator::merge_with_older_entries does (merge_operator.rs:341-435): operands are taken from the
newest link in batches of MERGE_BATCH_SIZE, each batch reversed to oldest first and merged with no existing value,
and the batch results, reversed to oldest first, are merged once with the base.

An operator is any object with merge_batch(key, existing, operands) -> bytes, where existing is bytes or None
and operands a list of bytes, oldest first (MergeOperator::merge_batch, merge_operator.rs:121-141).
"""
import numpy as np

from . import _abi

MERGE_BATCH_SIZE = 100  # merge_operator.rs:194


class StringConcat:
    """existing ++ operands in order: the reference's StringConcatMergeOperator (reader.rs:489) and
    MockMergeOperator (merge_operator.rs:504)."""

    @staticmethod
    def merge_batch(key, existing, operands):
        return (existing or b"") + b"".join(operands)


def fold(key, link_values_newest_first, base, operator):
    """The merged value of a chain.  link_values_newest_first: the operands' bytes; base: the base value's bytes,
    or None (no base, or a tombstone).  None when there is neither an operand nor a base
    (merge_operator.rs:427-430)."""
    links = list(link_values_newest_first)
    results = []
    for i in range(0, len(links), MERGE_BATCH_SIZE):  # process_batch (merge_operator.rs:341-359)
        results.append(operator.merge_batch(key, None, links[i:i + MERGE_BATCH_SIZE][::-1]))
    if not results and base is None:
        return None
    return operator.merge_batch(key, base, results[::-1])


def fold_chains(keys, res, sst_data, operator):
    """fold() over every item of a host copy of a merging read.  keys: the item's key (the queries of a get, the
    rows' keys of a scan); res: chain_start and the chain_sst / chain_val_off / chain_val_len / chain_flags
    columns as numpy arrays; sst_data: per SST of the tree its data section (uint8 array or bytes).  Returns, per
    item, the merged bytes, or None for an item without links."""
    cs = np.asarray(res["chain_start"]).astype(np.int64)
    out = []
    for i, key in enumerate(keys):
        vals, base = [], None
        for l in range(int(cs[i]), int(cs[i + 1])):
            vo, vl = int(res["chain_val_off"][l]), int(res["chain_val_len"][l])
            v = bytes(sst_data[int(res["chain_sst"][l])][vo:vo + vl])
            if int(res["chain_flags"][l]) & _abi.FLAG_MERGE_OPERAND:
                vals.append(v)
            else:
                base = v
        out.append(fold(key, vals, base, operator))
    return out


def fold_chains_mem(keys, res, table_vals, sst_data, operator):
    """fold_chains for a read over memtables and the tree (lsm_get_mem_device): a link whose chain_table is not
    0xFFFFFFFF reads its bytes from that table's value arena, table_vals[table] (uint8 array or bytes: sdb_run.val_base),
    at chain_val_off; any other link from sst_data[chain_sst], as in fold_chains."""
    cs = np.asarray(res["chain_start"]).astype(np.int64)
    out = []
    for i, key in enumerate(keys):
        vals, base = [], None
        for l in range(int(cs[i]), int(cs[i + 1])):
            vo, vl = int(res["chain_val_off"][l]), int(res["chain_val_len"][l])
            t = int(res["chain_table"][l]) & 0xFFFFFFFF
            src = table_vals[t] if t != 0xFFFFFFFF else sst_data[int(res["chain_sst"][l])]
            v = bytes(src[vo:vo + vl])
            if int(res["chain_flags"][l]) & _abi.FLAG_MERGE_OPERAND:
                vals.append(v)
            else:
                base = v
        out.append(fold(key, vals, base, operator))
    return out


def fold_scan_mem(res, table_vals, sst_data, operator):
    """fold_chains_mem over the rows of a scan over memtables and the tree (lsm_scan_mem_device with merge=True): the
    items are the output rows, keyed by their own keys (key_arena / key_off; summary[0] = num_entries), and a chain
    may run through tables and into the tree.  res: a host copy of the result.  Returns [(key, merged bytes)] in
    output order."""
    n = int(np.asarray(res["summary"])[0])
    ko = np.asarray(res["key_off"]).astype(np.int64)
    ka = np.asarray(res["key_arena"])
    keys = [ka[int(ko[i]):int(ko[i + 1])].tobytes() for i in range(n)]
    return list(zip(keys, fold_chains_mem(keys, res, table_vals, sst_data, operator)))
