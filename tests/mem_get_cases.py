"""Expected results of sdb_lsm_get_mem: device memtables in front of the tree of tests/get_cases.py.

MemTree restates rules M1-M5 of include/slatedb_amd.h literally (the reference: Reader::get_key_value_with_options,
reader.rs:133-182, over GetIterator::new, db_iter.rs:55-68, 102-124):
  M1  a key's chain is the tables in order, then the tree chain of get_cases.Tree;
  M2  a table is ordered key ascending, seq descending; it yields the rows with key == query and seq <= max_seq in
      table order; the first of them is the lower bound of (query, max_seq) in that order;
  M3  without a chain the first layer that yields an entry decides; a deciding table names (table, row), reports
      sst = NO_SST, block = 0 and the row's columns, and no SST was read or filtered;
  M4  with a chain the walk of merge_read_cases.get_merge runs across the layers: inside a table while rows are
      operands, into the next table, into the tree; sequence order is judged per table as it is per run;
  M5  a query that ends in the tables needs no block of the tree and sees none of its errors.
The tree part of a chain is get_merge's loop continued from the tables' state; with no tables get_merge() here
equals merge_read_cases.get_merge (tests/test_mem_get_cases.py holds them together).
"""
import collections

import numpy as np

from slatedb_amd import _abi, merge
from slatedb_amd.batch import Run

from . import get_cases as G
from . import merge_read_cases as M

U64_MAX = G.U64_MAX
NO_TABLE = 0xFFFFFFFF

# table / row: the deciding table row (NO_TABLE, 0: the tree decided, or nothing); tree: get_cases.Got of the tree
# part, None when a table decided; need: the tree blocks the query needs
MemGot = collections.namedtuple("MemGot", "state status table row tree need")
# links: ("t", table, row) or ("s", sst, row, block), newest first; first: the first entry, in the same terms
MemMGot = collections.namedtuple("MemMGot", "state status first links base ssts_read ssts_filtered cts ets need")


class Table:
    """One memtable as a sorted run.  entries: (key, kind, value, seq, create_ts, expire_ts), sorted here as
    KVTable keeps them.  rows: (key, val_off, val_len, seq, flags, create_ts | None, expire_ts | None), the tuples
    of scan_cases.Sst.rows; run: the batch.Run whose columns the device reads."""

    def __init__(self, entries):
        es = sorted(entries, key=lambda e: (e[0], -e[3]))
        assert len({(e[0], e[3]) for e in es}) == len(es), "a memtable holds one row per (key, seq)"
        self.run = r = Run.from_entries(es)
        self.rows = []
        for i, e in enumerate(es):
            flags = int(r.flags[i])
            self.rows.append((e[0], int(r.val_off[i]), int(r.val_len[i]), int(r.seq[i]), flags,
                              int(r.create_ts[i]) if flags & _abi.FLAG_HAS_CREATE_TS else None,
                              int(r.expire_ts[i]) if flags & _abi.FLAG_HAS_EXPIRE_TS else None))

    def yields(self, key, bound):
        """M2: the rows with key == query and seq <= bound, in table order."""
        out = [i for i, r in enumerate(self.rows) if r[0] == key and r[3] <= bound]
        # ... and the first of them is the lower bound of (query, bound) in (key ascending, seq descending) order
        lb = next((i for i, r in enumerate(self.rows) if r[0] > key or (r[0] == key and r[3] <= bound)), len(self.rows))
        assert (out[0] == lb) if out else (lb == len(self.rows) or self.rows[lb][0] != key)
        return out

    def value(self, i):
        _, vo, vl = self.rows[i][:3]
        return self.run.val_base[vo:vo + vl].tobytes()


def _state_of(flags, chain):
    if flags & _abi.FLAG_TOMBSTONE:
        return _abi.GET_DELETED, 0
    if flags & _abi.FLAG_MERGE_OPERAND:
        return _abi.GET_MERGE_OPERAND, 0 if chain else _abi.SDB_MERGE_OPERATOR_MISSING
    return _abi.GET_FOUND, 0


class MemTree:
    """tables: Tables in search order (the active memtable, then the immutable ones front first); tree: a
    get_cases.Tree, possibly without runs."""

    def __init__(self, tables, tree):
        self.tables, self.tree = list(tables), tree

    # -- M3 ----------------------------------------------------------------------------------------
    def get(self, key, max_seq=None):
        bound = U64_MAX if max_seq is None else int(max_seq)
        for t, table in enumerate(self.tables):
            ys = table.yields(key, bound)
            if ys:
                state, st = _state_of(table.rows[ys[0]][4], False)
                return MemGot(state, st, t, ys[0], None, set())
        g = self.tree.get(key, max_seq)
        return MemGot(g.state, g.status, NO_TABLE, 0, g, set(g.need))

    def columns(self, g):
        """The sdb_get_out columns plus table and row."""
        if g.tree is not None:
            z = self.tree.columns(g.tree)
        else:
            _, vo, vl, seq, flags, cts, ets = self.tables[g.table].rows[g.row]
            if flags & _abi.FLAG_TOMBSTONE:
                vo = vl = 0
            z = dict(state=g.state, status=g.status, sst=_abi.NO_SST, block=0, val_off=vo if vl else 0, val_len=vl, seq=seq,
                     flags=flags, create_ts=cts, expire_ts=ets, ssts_read=0, ssts_filtered=0)
        z.update(table=g.table, row=g.row)
        return z

    # -- M4 ----------------------------------------------------------------------------------------
    def row_of(self, link):
        return self.tables[link[1]].rows[link[2]] if link[0] == "t" else self.tree.leaves[link[1]].sst.rows[link[2]]

    def get_merge(self, key, max_seq=None):
        bound = U64_MAX if max_seq is None else int(max_seq)
        tree = self.tree
        read = filt = 0
        need = set()
        first, links, base, ended = None, [], False, False
        fail = lambda st: MemMGot(_abi.GET_NOT_FOUND, st, None, [], False, read, filt, None, None, need)  # noqa: E731
        newest = lambda: self.row_of(links[0])[3]  # noqa: E731

        def visit(link, r):  # -> True: the row ended the chain
            nonlocal first, base
            if first is None:
                first = link
            if r[4] & _abi.FLAG_TOMBSTONE:
                return True
            links.append(link)
            if not r[4] & _abi.FLAG_MERGE_OPERAND:
                base = True
                return True
            return False

        for t, table in enumerate(self.tables):
            top = 0
            for i in table.yields(key, bound):
                ended = visit(("t", t, i), table.rows[i])
                if table.rows[i][4] & _abi.FLAG_TOMBSTONE:
                    break
                top = max(top, table.rows[i][3])
                if ended:
                    break
            if links and top > newest():
                return fail(_abi.SDB_INVALID_SEQUENCE_ORDER)
            if ended:
                break
        i0 = 0
        for run in ([] if ended else tree.runs):  # merge_read_cases.get_merge's loop, from the tables' state on
            err, top = 0, 0
            for i in range(i0, i0 + len(run)):
                l = tree.leaves[i]
                if not l.covers(key):
                    continue
                what, (bs, be) = tree.step(i, key)
                if what == "filtered":
                    filt += 1
                    continue
                if what is not None:
                    err = what
                    break
                if be <= bs:
                    continue
                read += 1
                need |= {int(tree.block_base[i]) + b for b in range(bs, be)}
                bad = [l.block_status[b] for b in range(bs, be) if l.block_status.get(b)]
                if bad:
                    err = bad[0]
                    break
                s = l.sst
                for e in range(s.bes[bs], s.bes[be]):
                    r = s.rows[e]
                    if r[0] != key or r[3] > bound:
                        continue
                    ended = visit(("s", i, e, M._block_of(s, bs, be, e)), r)
                    if r[4] & _abi.FLAG_TOMBSTONE:
                        break
                    top = max(top, r[3])
                    if ended:
                        break
                if ended:
                    break
            i0 += len(run)
            if links and top > newest():
                return fail(_abi.SDB_INVALID_SEQUENCE_ORDER)
            if err:
                return fail(err)
            if ended:
                break
        if first is None:
            return MemMGot(_abi.GET_NOT_FOUND, 0, None, [], False, read, filt, None, None, need)
        flags = self.row_of(first)[4]
        if flags & _abi.FLAG_TOMBSTONE:
            return MemMGot(_abi.GET_DELETED, 0, first, [], False, read, filt, None, None, need)
        cts, ets = M._fold_ts([self.row_of(l) for l in links], None, None)
        return MemMGot(_state_of(flags, True)[0], 0, first, links, base, read, filt, cts, ets, need)

    def merge_columns(self, g):
        """The per-query columns of a chained get, plus table and row."""
        z = dict(state=g.state, status=g.status, sst=_abi.NO_SST, block=0, val_off=0, val_len=0, seq=0, flags=0,
                 create_ts=None, expire_ts=None, ssts_read=g.ssts_read, ssts_filtered=g.ssts_filtered, table=NO_TABLE, row=0)
        if g.first is None:
            return z
        _, vo, vl, seq, flags, cts, ets = self.row_of(g.first)
        if g.first[0] == "t":
            z.update(table=g.first[1], row=g.first[2])
        else:
            z.update(sst=g.first[1], block=g.first[3])
        if flags & _abi.FLAG_TOMBSTONE:
            z.update(seq=seq, flags=flags, create_ts=cts, expire_ts=ets)
        else:
            z.update(val_off=vo if vl else 0, val_len=vl, seq=seq, flags=M.agg_flags(g.base, g.cts, g.ets), create_ts=g.cts,
                     expire_ts=g.ets)
        return z

    def link_columns(self, link):
        _, vo, vl, seq, flags, cts, ets = self.row_of(link)
        z = dict(val_off=vo if vl else 0, val_len=vl, seq=seq, flags=flags, create_ts=cts, expire_ts=ets)
        if link[0] == "t":
            z.update(sst=_abi.NO_SST, block=0, table=link[1], row=link[2])
        else:
            z.update(sst=link[1], block=link[3], table=NO_TABLE, row=0)
        return z

    def link_bytes(self, link):
        if link[0] == "t":
            return self.tables[link[1]].value(link[2])
        _, vo, vl = self.row_of(link)[:3]
        return self.tree.leaves[link[1]].sst.data[vo:vo + vl].tobytes()

    def folded(self, key, g):
        """merge.fold over a chain's bytes; None for a query without links."""
        if not g.links:
            return None
        vals = [self.link_bytes(l) for l in g.links]
        return merge.fold(key, vals[:-1] if g.base else vals, vals[-1] if g.base else None, M.OP)

    def covering_blocks(self, key, max_seq=None, chain=False):
        """What an eager call may check for a query: nothing once the tables end it (M5), else the tree's."""
        return set() if self.ends_in_tables(key, max_seq, chain) else self.tree.covering_blocks(key)

    def ends_in_tables(self, key, max_seq=None, chain=False):
        """M5: without a chain a table yields an entry; with a chain a value or tombstone in a table ends it."""
        bound = U64_MAX if max_seq is None else int(max_seq)
        for table in self.tables:
            for i in table.yields(key, bound):
                if not chain or not table.rows[i][4] & _abi.FLAG_MERGE_OPERAND:
                    return True
        return False


def is_table_layer(name):
    return name == "mem" or name.startswith("imm")


def golden_mem_tree(case, version, block_size=4096, bloom=False):
    """A golden case (get_cases.json, or a get case of merge_read_cases.json) with its mem / imm<i> layers as
    tables and the rest as runs of one SST, in the fixture's layer_order."""
    tables, runs, seen_sst = [], [], False
    for layer in case["layer_order"]:
        es = [(e["key"].encode(), e["kind"], e["value"].encode(), e["seq"], None, e["expire_ts"])
              for e in case["entries"] if e["layer"] == layer]
        if is_table_layer(layer):
            assert not seen_sst, "the memtables come before the tree"
            tables.append(Table(es))
        else:
            seen_sst = True
            runs.append([G.leaf_of(es, version, block_size, bloom)])
    return MemTree(tables, G.Tree(runs))


def value_of(mt, cols):
    """The value bytes a get's columns name."""
    vo, vl = cols["val_off"], cols["val_len"]
    if cols["table"] != NO_TABLE:
        return mt.tables[cols["table"]].run.val_base[vo:vo + vl].tobytes()
    return mt.tree.leaves[cols["sst"]].sst.data[vo:vo + vl].tobytes()


def host_tables(tables):
    return [np.asarray(t.run.val_base) for t in tables]
