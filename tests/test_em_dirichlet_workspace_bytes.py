"""CPU: tclip_workspace_bytes and tclip_em_dirichlet_until_stable_workspace_bytes return, for every problem of the grid below,
the sizes recorded in tests/golden/em_dirichlet_workspace_bytes.json.  The record was taken from the library of the commit
before the host driver got its one workspace view (scripts/build_rev_variant.sh, loaded through TCLIP_LIB): the view, the
group split and both queries must keep every size, byte for byte.

    TCLIP_LIB=variants/<name>.so python tests/test_em_dirichlet_workspace_bytes.py --record      # rewrites the golden file
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "transductive-clip_amd"))
from tclip_amd import _capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "em_dirichlet_workspace_bytes.json")
CLASSES = (2, 100, 397, 1000)
BATCHES = ((1, 1), (3, 4), (10, 20), (17, 5))        # (n_batches, tasks_per_batch): one, one, three, two stream groups at K = 100
QUERIES = (10, 75)
ITER_MM = (1, 50, 51, 101, 1000)                     # the edges of the chunk and checkpoint counts
# problems check_problem refuses: both queries return 0
INVALID = ((0, 1, 75, 100, 0, 10, 1000, 1, 0), (1, 0, 75, 100, 0, 10, 1000, 1, 0), (1, 1, 0, 100, 0, 10, 1000, 1, 0),
           (1, 1, 75, 1, 0, 10, 1000, 1, 0), (1, 1, 75, 1025, 0, 10, 1000, 1, 0), (1, 1, 75, 100, -1, 10, 1000, 1, 0),
           (1, 1, 75, 100, 16001, 10, 1000, 1, 0), (1, 1, 75, 100, 0, -1, 1000, 1, 0), (1, 1, 75, 100, 0, 10, 0, 1, 0),
           (256, 256, 75, 100, 0, 10, 1000, 1, 0))


def _grid():
    """every problem as the nine fields of tclip_problem, in the order of the golden file"""
    for few_shot, K, (B, N), Q, iter_mm in itertools.product((False, True), CLASSES, BATCHES, QUERIES, ITER_MM):
        yield (B, N, Q, K, 2 * K if few_shot else 0, 10, iter_mm, K, 1 if few_shot else 0)
    yield from INVALID


def _sizes():
    lib = _capi.lib()
    out = []
    for fields in _grid():
        p = _capi.Problem(*fields)
        out.append([int(lib.tclip_workspace_bytes(ctypes.byref(p))),
                    int(lib.tclip_em_dirichlet_until_stable_workspace_bytes(ctypes.byref(p)))])
    return out


def test_workspace_bytes_are_the_recorded_ones():
    if os.environ.get("TCLIP_STREAM_GROUPS") or os.environ.get("TCLIP_GROUP_SIZES"):
        pytest.skip("TCLIP_STREAM_GROUPS / TCLIP_GROUP_SIZES change the group split the record was taken with")
    golden = json.load(open(GOLDEN))
    problems = [list(f) for f in _grid()]
    assert golden["problems"] == problems                 # the record covers exactly this grid
    got = _sizes()
    assert len(got) == len(golden["bytes"]) == 2 * 4 * 4 * 2 * 5 + len(INVALID)
    wrong = [(f, g, w) for f, g, w in zip(problems, got, golden["bytes"]) if g != w]
    assert not wrong, wrong[:5]
    n_valid = len(got) - len(INVALID)
    assert all(plain > 0 and stable > plain for plain, stable in got[:n_valid])
    assert all(pair == [0, 0] for pair in got[n_valid:])


if __name__ == "__main__" and "--record" in sys.argv:
    json.dump({"fields": [n for n, _ in _capi.Problem._fields_], "problems": [list(f) for f in _grid()], "bytes": _sizes()},
              open(GOLDEN, "w"), separators=(",", ":"))
    print("wrote", GOLDEN)
