"""Records tests/golden/kat_cycleforest.json: what the CPU restatement of the closed-trail search gives, per map, for every (set, order)
of tests/cycleforest_ref.py -- the figures tests/test_gpu_cycleforest.py holds liblle_cycleforest.so to, so that no GPU test walks a
search in Python.

    python -m tests.golden.make_kat_cycleforest            # every set
    python -m tests.golden.make_kat_cycleforest T M        # some sets (the others keep what the file has)

Per set and order a list with one entry per map: `length` (null: no plan within the set's t_max), `frontier` and `expanded` per depth
and `states` (distinct records stored), from `cycles_ref.search` under the map's `changes`.  Where an embedded map is an unchanged map
of tests/golden/kat_cycles.json at the same t_max and order, the figures must be those recorded there: asserted here.  So are the
figures tests/cycleforest_ref.py states.
"""
import json
import os
import sys
import time

from tests import cycleforest_ref

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_cycleforest.json")


def record(s):
    out = {}
    for order in s.orders:
        rows = []
        for m in range(len(s.maps)):
            row = cycleforest_ref.row_of(cycleforest_ref.search(s, m, order))
            single = cycleforest_ref.single_search(s.base[m], s.t_max, order) if s.changes[m] is None else None
            assert single is None or single == row, (s.name, s.names[m], order, single, row)
            want = cycleforest_ref.STATED.get((s.name, s.names[m], order))
            assert want is None or want == (row["length"], row["states"]), (s.name, s.names[m], order, want, row["length"], row["states"])
            rows.append(row)
        out[str(order)] = rows
    return out


def main(names):
    golden = {}
    if os.path.exists(PATH):
        with open(PATH) as f:
            golden = json.load(f)
    for name in names or sorted(cycleforest_ref.SETS):
        t0 = time.time()
        golden[name] = record(cycleforest_ref.SETS[name])
        print(f"set {name}: {time.time() - t0:.1f} s", flush=True)
    with open(PATH, "w") as f:
        json.dump(golden, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
