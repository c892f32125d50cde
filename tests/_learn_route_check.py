"""Run as a subprocess by tests/test_gpu_learn_routes.py (the library reads its EC_* switches once per process, so the cases of
a switch setting need a process that starts under it): runs the named cases of tests/_learn_route_cases.py on cuda:0 and
prints one JSON line per case -- the error figures of the outputs and of every gradient tensor against the float64 oracle,
whether a second run in a fresh workspace gave the same bits, and the worst rel-L2 between the two runs.  Stops at the first
case that raises (non-zero exit)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _learn_route_ref as ref  # noqa: E402


def main(names):
    dev = torch.device("cuda:0")
    for name in names:
        case = ref.cases.CASES[name]
        want = ref.cases.SETTINGS[case["env"]]
        assert {k: os.environ.get(k) for k in want} == want, (name, want)
        r = ref.run_case(name, dev)
        print(json.dumps({"case": name, "figs": r["figs"], "equal": r["equal"], "rerun": r["rerun"], "nohf_equal": r.get("nohf_equal")}),
              flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
