"""Worker of tests/test_score_exact_gpu.py::test_exit_schedules: runs the trip-edge batches
(tests/exact_cases.py TripCase) through score_batch, plain and with the exact early exit,
in a fresh process -- the engine reads MADPOSE_SCORE_CHECK and MADPOSE_SCORE_PAIR once per
process -- and prints the results as exact hex floats / integers, one JSON line.
Arguments: variant, then the sizes n."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import exact_cases as xc  # noqa: E402


def main():
    variant = int(sys.argv[1])
    out = {}
    for n in (int(a) for a in sys.argv[2:]):
        r = xc.run_trip_case(xc.trip_case(n, variant))
        out[str(n)] = {"plain": [float(v).hex() for v in r["plain"]], "exit": [float(v).hex() for v in r["exit"]],
                       "plain_slot": [int(v) for v in r["plain_slot"]], "exit_slot": [int(v) for v in r["exit_slot"]],
                       "best": float(r["best"]).hex(), "tie": [float(v).hex() for v in r["tie"]]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
