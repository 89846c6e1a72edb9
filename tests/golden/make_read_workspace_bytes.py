"""Generate tests/golden/read_workspace_bytes.json: what the ten sdb_lsm_*_workspace_bytes functions of the built
library return over a small grid.  The sizes are part of the C contract (a caller may have allocated by them), so
the fixture is recorded once and tests/test_read_workspace_bytes.py holds every later build to it.

Run with the library built; the sizers need no device:

    python tests/golden/make_read_workspace_bytes.py          # writes the fixture
    python tests/golden/make_read_workspace_bytes.py --check  # compares with the committed fixture

Each list in "sizes" is in the order of itertools.product over the grid axes named in "axes" for that function.
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
OUT = os.path.join(HERE, "read_workspace_bytes.json")

GRID = {"total_blocks": [0, 1, 7, 1025], "num_ssts": [0, 1, 5], "num_runs": [0, 1, 3], "n": [0, 1, 1023, 1025],
        "cand": [[0, 0], [16, 256], [1025, 40000]], "merge": [0, 1], "num_tables": [0, 1, 3]}
TREE = ("total_blocks", "num_ssts", "num_runs", "n")
AXES = {"sdb_lsm_get_workspace_bytes": TREE,
        "sdb_lsm_get_merge_workspace_bytes": TREE,
        "sdb_lsm_get_filtered_workspace_bytes": TREE + ("merge",),
        "sdb_lsm_scan_workspace_bytes": TREE + ("cand",),
        "sdb_lsm_scan_merge_workspace_bytes": TREE + ("cand",),
        "sdb_lsm_scan_filtered_workspace_bytes": TREE + ("cand", "merge"),
        "sdb_lsm_get_projected_workspace_bytes": TREE + ("merge",),
        "sdb_lsm_get_mem_workspace_bytes": ("num_tables",) + TREE + ("merge",),
        "sdb_lsm_scan_projected_workspace_bytes": TREE + ("cand", "merge"),
        "sdb_lsm_scan_mem_workspace_bytes": ("num_tables",) + TREE + ("cand", "merge")}


def sizes(lib):
    """{function: [its value at every grid point]} of the loaded library."""
    out = {}
    for name, axes in AXES.items():
        fn = getattr(lib, name)
        vals = []
        for point in itertools.product(*[GRID[a] for a in axes]):
            args = []
            for x in point:
                args.extend(x if isinstance(x, list) else [x])
            vals.append(int(fn(*args)))
        out[name] = vals
    return out


def main():
    from slatedb_amd import runtime
    data = {"grid": GRID, "axes": {k: list(v) for k, v in AXES.items()}, "sizes": sizes(runtime.lib())}
    total = sum(len(v) for v in data["sizes"].values())
    if "--check" in sys.argv:
        if json.load(open(OUT)) != data:
            sys.exit("read_workspace_bytes.json differs from the built library")
        print("read_workspace_bytes.json matches the built library (%d sizes)" % total)
        return
    json.dump(data, open(OUT, "w"), separators=(",", ":"))
    print("wrote %s (%d sizes)" % (OUT, total))


if __name__ == "__main__":
    main()
