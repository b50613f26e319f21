#!/usr/bin/env python3
"""Generate tests/golden/plan_layout.json: what lnx_plan_create lays out for every configuration of tests/plan_layout_cases.py.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen/make_plan_layout.py

Needs the built library and no GPU.  Run it on the commit whose layout is to be kept: the fixture is the record a later change of
linnaeus_amd/csrc/plan.cpp is compared with, so regenerating it is a statement that the layout was meant to change."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.abspath(os.path.join(HERE, "..", "..", ".."))
sys.path.insert(0, REPO)
sys.dont_write_bytecode = True

from tests.plan_layout_cases import CONFIGS, measure  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "plan_layout.json")

if __name__ == "__main__":
    # one configuration per line keeps the file small and a changed configuration one line of diff
    lines = [f"{json.dumps(name)}: {json.dumps(measure(name), separators=(',', ':'))}" for name in CONFIGS]
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(lines) + "\n}\n")
    print(f"wrote {OUT}: {len(lines)} configurations, {os.path.getsize(OUT)} bytes")
