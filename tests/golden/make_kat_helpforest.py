"""Records tests/golden/kat_helpforest.json: what the CPU restatements of the two searches give, per map, for every (set, mode, param)
of tests/helpforest_ref.py -- the figures tests/test_gpu_helpforest.py holds liblle_helpforest.so to, so that no GPU test walks a
search in Python.

    python -m tests.golden.make_kat_helpforest            # every set
    python -m tests.golden.make_kat_helpforest S P        # some sets (the others keep what the file has)

Per set and "mode/param" a list with one entry per map: `length` (null: no plan within the set's t_max), `frontier` and `expanded` per
depth and `states` (distinct records stored), from `helpgraph_ref.search` (modes over the flattened help relation) or
`trails_ref.search` (no-sequence-N), with the set's collect_gems and the map's `changes` (sets L and C).  Nothing is trimmed: every set has the maps, the t_max and the
shape tests/helpforest_ref.py states.
"""
import json
import os
import sys
import time

from tests import helpforest_ref

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kat_helpforest.json")


def record(s):
    out = {}
    for mode, param in s.modes:
        rows = []
        for text, changes in zip(s.maps, s.changes):
            r = helpforest_ref.search(text, s.t_max, mode, param, s.collect_gems, changes=changes)
            rows.append(dict(length=r.length, frontier=list(r.frontier), expanded=list(r.expanded), states=r.n_states))
        out[helpforest_ref.golden_key(mode, param)] = rows
    return out


def main(names):
    golden = {}
    if os.path.exists(PATH):
        with open(PATH) as f:
            golden = json.load(f)
    for name in names or sorted(helpforest_ref.SETS):
        t0 = time.time()
        golden[name] = record(helpforest_ref.SETS[name])
        print(f"set {name}: {time.time() - t0:.1f} s", flush=True)
    with open(PATH, "w") as f:
        json.dump(golden, f, indent=None, separators=(",", ":"), sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1:])
