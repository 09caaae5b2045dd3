"""Records what mrec_sparse_apply_workspace_bytes answers over a grid of (n, D) as tests/golden/apply_ws_bytes.json.

The query is pure host code (no device needed).  The fixture pins the sizes callers were promised: tests/test_apply_workspace.py
holds every later build to them, so regenerate it only where a change of the workspace's size is the point of the change.

Run from the repo root, with the library built:  python tests/golden/make_apply_ws_bytes.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from mindrec_amd import _lib  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
NS = [0, 1, 8, 9, 64, 65, 4096, 638976]
DS = [1, 4, 30, 80, 84, 252, 256, 260, 1024]


def main():
    table = [[_lib.query_bytes("mrec_sparse_apply_workspace_bytes", n, d) for d in DS] for n in NS]
    with open(os.path.join(HERE, "apply_ws_bytes.json"), "w") as f:
        json.dump({"n": NS, "D": DS, "bytes": table}, f)
        f.write("\n")


if __name__ == "__main__":
    main()
