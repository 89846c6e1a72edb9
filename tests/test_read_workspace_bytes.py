"""The sizes the ten sdb_lsm_*_workspace_bytes functions return are part of the C contract: callers allocate by
them.  tests/golden/read_workspace_bytes.json holds them over a small grid as recorded before the get's two binds and
sizers were folded into one, those of the _projected and _mem functions as recorded before the launchers took one call
descriptor (tests/golden/make_read_workspace_bytes.py); every build returns exactly those.  The sizers need no device."""
import itertools
import json
import os

import pytest

from slatedb_amd import runtime

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "read_workspace_bytes.json")))


def test_grid_is_the_agreed_one():
    g = GOLDEN["grid"]
    assert g["total_blocks"] == [0, 1, 7, 1025] and g["num_ssts"] == [0, 1, 5] and g["num_runs"] == [0, 1, 3]
    assert g["n"] == [0, 1, 1023, 1025] and g["cand"] == [[0, 0], [16, 256], [1025, 40000]] and g["merge"] == [0, 1]
    assert g["num_tables"] == [0, 1, 3]
    assert sorted(GOLDEN["sizes"]) == sorted("sdb_lsm_%s%s_workspace_bytes" % (f, v) for f in ("get", "scan")
                                             for v in ("", "_merge", "_filtered", "_projected", "_mem"))
    for name, axes in GOLDEN["axes"].items():
        assert (axes[0] == "num_tables") == name.endswith("_mem_workspace_bytes"), name


@pytest.mark.parametrize("name", sorted(GOLDEN["sizes"]))
def test_workspace_bytes_are_the_recorded_ones(name):
    fn = getattr(runtime.lib(), name)
    points = list(itertools.product(*[GOLDEN["grid"][a] for a in GOLDEN["axes"][name]]))
    want = GOLDEN["sizes"][name]
    assert len(points) == len(want)
    for point, size in zip(points, want):
        args = [y for x in point for y in (x if isinstance(x, list) else [x])]
        assert int(fn(*args)) == size, (name, args)
