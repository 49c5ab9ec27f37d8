#!/usr/bin/env python3
"""Record tests/data/sweep_plans.json: the launch plan of every case of
tests/test_gpu_sweep_plan.py from the library as built (needs the GPU).

Run it on the commit whose plans are to be pinned -- before a change of the
planners that is meant to keep them -- and commit the file with that change:

    python scripts/record_sweep_plans.py [--commit REV] [--out FILE]

--commit is written into the file as the commit that produced it (default:
`git rev-parse HEAD` when the tree is a git checkout)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: F401,E402  (one HIP runtime for torch and the engine, as in tests/conftest.py)

import test_gpu_sweep_plan as plan  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=plan.TABLE)
    a = ap.parse_args()
    commit = a.commit
    if commit is None:
        try:
            commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], check=True,
                                    capture_output=True, text=True).stdout.strip()
        except (OSError, subprocess.CalledProcessError):
            commit = "unknown"
    plans = {}
    for case in sorted(plan.CASES):
        knobs = plan.CASES[case][2]
        saved = {k: os.environ.get(k) for k in knobs}
        os.environ.update(knobs)
        try:
            plans[case] = plan.record(case)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        print(f"{case}: {plans[case]['mode']}, {plans[case]['n_launches']} launches, "
              f"{plans[case]['device_bytes']} device bytes", flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump({"recorded_from_commit": commit, "plans": plans}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
