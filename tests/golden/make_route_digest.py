"""Writes tests/golden/route_digest.json: the digest (tests/routedigest.py) of the model ``train_ddp.Solver`` builds from every config
under every setting of ``routedigest.SETTINGS``, as the checked-out commit routes it.  Run from the repository root of the commit whose
routing is the reference -- for a refactoring of the routing that is the PARENT commit, with this file and tests/routedigest.py
copied in:

    python tests/golden/make_route_digest.py [output path]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "ssds.pytorch_amd"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import routedigest  # noqa: E402


def main(path):
    out = {}
    for cfg_name in routedigest.configs():
        for setting in routedigest.SETTINGS:
            out["%s/%s" % (cfg_name, setting)] = routedigest.digest(routedigest.canonical(cfg_name, setting))
        print(cfg_name, len(routedigest.SETTINGS), "settings")
    with open(path, "w") as f:  # one key per line: a change of one build is one line of a diff
        f.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in out.items()) + "\n}\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "route_digest.json"))
