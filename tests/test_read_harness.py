"""tests/read_harness.py on CPU tensors: the guard bytes and the pre-filled outputs see a byte that changed, and host()
decodes the result dict of each read family."""
import numpy as np
import pytest
import torch

from slatedb_amd import runtime

from .read_harness import Filled, Guard, host, untouched

U64_MAX = (1 << 64) - 1


def test_guard_sees_a_byte_before_or_after_an_array():
    for where in (None, "before", "after"):
        guard = Guard("cpu")
        a = guard("seq", 5, torch.int64, 0)
        ws = guard("_ws", 33, torch.uint8, None)
        assert a.numel() == 5 and a.dtype == torch.int64 and ws.numel() == 33 and ws.data_ptr() % 2 == 1
        assert guard("key_arena", 0, torch.uint8, 0).numel() == 0
        a.fill_(7)  # what a call writes inside its arrays is its own
        ws.fill_(7)
        big, lead, nb = guard.bufs[0]
        assert nb == 40 and big.data_ptr() + lead == a.data_ptr()
        if where == "before":
            big[lead - 1] = 0
        elif where == "after":
            big[lead + nb] = 0
        if where is None:
            guard.check()
        else:
            with pytest.raises(AssertionError):
                guard.check()


def test_filled_and_untouched_see_one_changed_byte():
    new = Filled(0xA5, "cpu")
    res = {"seq": new("seq", 4, torch.int64, 0), "key_arena": new("key_arena", 10, torch.uint8, 0),
           "chain_flags": new("chain_flags", 3, torch.uint8, 0x5A), "range_status": new("range_status", 2, torch.int32, 0),
           "key_off": new("key_off", 5, torch.int64, 0), "chain_start": new("chain_start", 5, torch.int64, 0),
           "summary": new("summary", 7, torch.int64, 0), "range_entry_start": new("range_entry_start", 0, torch.int64, 0)}
    # room behind the capacity for the columns and the keys, none for what a test reads whole
    assert {k: v.numel() for k, v in res.items()} == {"seq": 12, "key_arena": 74, "chain_flags": 11, "range_status": 2,
                                                      "key_off": 5, "chain_start": 5, "summary": 7, "range_entry_start": 1}
    h = {k: v.numpy() for k, v in res.items()}
    assert untouched(h, list(h), 0xA5)
    h["seq"].view(np.uint8)[13] ^= 1  # one byte inside a column
    assert not untouched(h, ["seq"], 0xA5) and untouched(h, [k for k in h if k != "seq"], 0xA5)
    assert not untouched(h, list(h), 0xA5)


def words(*values):
    return torch.tensor([v - (1 << 64) if v >= 1 << 63 else v for v in values], dtype=torch.int64)


def test_host_decodes_each_family():
    inv = runtime._abi.SDB_INVALID_ARGUMENT
    get = {"state": torch.tensor([1, 0], dtype=torch.uint8), "summary": words(1, 2, 3, 4, 5, U64_MAX, inv), "_ws": None}
    h = host(get)
    assert set(h) == {"state", "summary"} | {"sum_" + f for f in runtime.GET_SUMMARY}
    assert [h["sum_" + f] for f in runtime.GET_SUMMARY] == [1, 2, 3, 4, 5, U64_MAX, inv] and h["state"].tolist() == [1, 0]
    chain = dict(get, chain_start=words(0, 1, 1), chain_summary=words(9, 4, (0xFFFFFFFF << 32) | inv))
    h = host(chain)
    assert [h["csum_" + f] for f in runtime.CHAIN_SUMMARY] == [9, 4, inv] and h["sum_num_found"] == 1
    scan = {"range_entry_start": words(0, 2), "summary": words(2, 10, 3, 15, 0, 6, 0)}
    h = host(scan)
    assert [h["sum_" + f] for f in runtime.LSM_SCAN_SUMMARY] == [2, 10, 3, 15, 0, 6, 0]
    assert "sum_num_filtered" not in h and "csum_num_links" not in h
    h = host(dict(scan, num_filtered=words(12), range_filtered=torch.zeros(1, dtype=torch.int32),
                  chain_summary=words(5, 2, 0), range_sources_read=torch.ones(1, dtype=torch.int32)))
    assert h["sum_num_filtered"] == 12 and h["csum_num_links"] == 5 and h["sum_num_candidates"] == 3
    assert h["range_sources_read"].tolist() == [1]
