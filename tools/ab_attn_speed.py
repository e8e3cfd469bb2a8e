#!/usr/bin/env python3
"""Compare two builds of the library on the key-tiled attention benchmarks: per (case, direction), B's best round may exceed A's
by no more than A's own round-to-round spread (slowest / fastest round - 1) in the same session.

    python tools/ab_attn_speed.py DIR

DIR holds the --out files of runs that alternated A and B on one machine (MV_LIB_PATH selects the build):
    long_A.txt  long_B.txt    tools/bench_attn_long.py
    half_A.txt  half_B.txt    tools/bench_attn_long.py --half
    dh_A.txt    dh_B.txt      tools/bench_attn_dh.py
Prints one line per pair; exit status 0 when every pair is inside the bound, 1 otherwise."""
import json
import os
import sys


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    d = sys.argv[1]
    ok = True
    for tool, arms in (("long", ("long_fwd", "long_bwd")), ("half", ("long_fwd", "long_bwd")), ("dh", ("dh_fwd", "dh_bwd"))):
        def load(w):
            return [json.loads(l) for l in open(os.path.join(d, f"{tool}_{w}.txt")) if l.startswith("{")]
        A, B = load("A"), load("B")
        assert len(A) == len(B), f"{tool}: {len(A)} cases from A, {len(B)} from B"
        for a, b in zip(A, B):
            assert (a.get("dim_head"), a["B"], a["N"]) == (b.get("dim_head"), b["B"], b["N"]), f"{tool}: case mismatch {a} / {b}"
            for arm in arms:
                ta, tb, sa = a[arm + "_us"], b[arm + "_us"], a[arm + "_spread"]
                good = tb <= ta * (1 + sa)
                ok &= good
                print(f"{tool:5s} dh={a.get('dim_head', 64):3d} B={a['B']:3d} N={a['N']:5d} {arm:9s} A {ta:9.1f} us (spread {100 * sa:5.2f} %, "
                      f"B's {100 * b[arm + '_spread']:5.2f} %)  B {tb:9.1f} us  {100 * (tb / ta - 1):+6.2f} %  {'ok' if good else 'SLOWER'}")
    print("every pair inside A's spread" if ok else "some pairs outside A's spread")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
