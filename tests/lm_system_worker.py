"""Worker of tests/test_lm_system_cpu.py::test_switches_do_not_change_the_host_lm: the
host LM (mp_debug_lm_refine_host) on one 2049-block and one 300-block problem in a fresh
process -- the pool size, the wide threshold and the ISA choice are read once per process
(MADPOSE_LO_THREADS, MADPOSE_LM_WIDE, MADPOSE_LM_ISA) -- printing the refined models'
doubles as hex and the statuses, one JSON line."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import madpose  # noqa: E402
from tests import lm_system_cases as SC  # noqa: E402


def main():
    cx = SC.big(0)
    rng = np.random.default_rng(77)
    specs = [SC.spec(rng, cx, (683, 683, 683)), SC.spec(rng, cx, (100, 100, 100))]
    got = madpose.lm_refine_batch(0, *cx.args, cx.o, SC.config_of(specs[0]),
                                  [(s.kind, s.lists, s.model) for s in specs], on_host=True)
    out = []
    for m, st in got:
        R, t, sc, o0, o1, _, _ = SC.model_doubles(m, 0)
        out.append({"model": [float(v).hex() for v in R + t + [sc, o0, o1]], "status": int(st)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
