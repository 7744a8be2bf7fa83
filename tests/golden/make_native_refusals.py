"""Fixture native_refusals.json: what every case of tests/test_native_refusals_host.py raises, class name and full message, recorded
from the binding at the commit BEFORE its call path, workspace and tensor checks were folded into one place each.  Needs the built
library and no GPU:

    python tests/golden/make_native_refusals.py

Run it only at a commit whose refusals are the ones to keep: after a refactor of the binding the fixture is the yardstick, and a
message that differs is the refactor's mistake.  Every case must raise (checked here); the file is written sorted, one case a line.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_native_refusals_host as T  # noqa: E402


def main():
    out = {}
    for cid, (fn, kwargs) in sorted(T.CASES.items()):
        kind, text = T.refusal(fn, kwargs)
        assert kind is not None, f"{cid}: the call returned; every case must be refused on a CPU"
        out[cid] = {"type": kind, "message": text}
    with open(T.FIXTURE, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in out.items()) + "\n}\n")
    kinds = sorted({v["type"] for v in out.values()})
    print(f"{len(out)} cases of {len(T.WELL_FORMED)} wrappers -> {T.FIXTURE} ({os.path.getsize(T.FIXTURE)} bytes); classes: {kinds}")


if __name__ == "__main__":
    main()
