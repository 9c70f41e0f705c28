"""Writes tests/golden/plan_digest.json: the digest (tests/plandigest.py) of every plan of ``plandigest.PLANS`` as the checked-out
commit records it.  Run from the repository root of the commit whose recordings are the reference -- for a refactoring of the plan's
Python side that is the PARENT commit, with this file and tests/plandigest.py copied in:

    python tests/golden/make_plan_digest.py [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import plandigest  # noqa: E402


def main(path):
    models, out = {}, {}
    for key in plandigest.PLANS:
        canon, _ = plandigest.record(key, models)
        out[key] = canon if "unsupported" in canon else plandigest.digest(canon)
        print(key, len(out[key].get("ops", ())), "ops")
    with open(path, "w") as f:  # one plan per line: a change of one plan is one line of a diff
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "plan_digest.json"))
