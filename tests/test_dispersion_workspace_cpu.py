"""CPU: the workspace queries of the dispersion families (csrc/dispersion.hip behind dlsa_gamma_workspace_bytes and
dlsa_tweedie_workspace_bytes) return, for every argument of the grid below, the number they returned before the Gamma and Tweedie
layouts became one -- tests/golden/dispersion_workspace_queries.json, written by `python tests/test_dispersion_workspace_cpu.py
--record FILE` in a checkout built at the commit before that change.  The queries are host-only arithmetic; the structured
one-hot queries need a plan, which cannot be created without a device (bench/ab_dispersion_entries.py compares those)."""
import itertools
import json
import os
import sys

MAX_ROWS = (0, 1, 255, 256, 257, 700, 100000)
P = (1, 5, 64, 121, 500, 2047)
INTERCEPT = (0, 1)
ROW_STEP = (1, 3)
# (max_rows, p, intercept, row_step): p = 0, pe > 2048 (with and through the intercept), row_step = 0, max_rows < 0
REFUSED = ((700, 0, 0, 1), (700, 0, 1, 1), (700, 2049, 0, 1), (700, 2048, 1, 1), (700, 5, 1, 0), (-1, 5, 1, 1))
QUERIES = ("dlsa_gamma_workspace_bytes", "dlsa_tweedie_workspace_bytes")
GOLDEN_NAME = "dispersion_workspace_queries.json"


def cases():
    return list(itertools.product(MAX_ROWS, P, INTERCEPT, ROW_STEP)) + list(REFUSED)


def record(lib):
    """{query: [[max_rows, p, intercept, row_step, bytes], ...]} over cases()"""
    return {q: [[*c, int(getattr(lib, q)(*c))] for c in cases()] for q in QUERIES}


def test_queries_equal_the_recorded_ones():
    from conftest import golden_path
    from dlsa_amd import _lib
    want = json.load(open(golden_path(GOLDEN_NAME)))
    got = record(_lib.load())
    assert sorted(want) == sorted(QUERIES)
    for q in QUERIES:
        assert len(want[q]) == len(cases()) == 7 * 6 * 2 * 2 + len(REFUSED)
        assert got[q] == want[q], [(g, w) for g, w in zip(got[q], want[q]) if g != w][:5]


def test_the_record_is_not_trivial():
    """refusals are 0, everything else is a positive multiple of 256, the strided query is never the smaller one, and the two
    families differ by Tweedie's fourth once-per-partition sum (1024 doubles)"""
    from conftest import golden_path
    want = json.load(open(golden_path(GOLDEN_NAME)))
    for q in QUERIES:
        rows = {tuple(r[:4]): r[4] for r in want[q]}
        assert all(rows[c] == 0 for c in REFUSED)
        for m, p, i in itertools.product(MAX_ROWS, P, INTERCEPT):
            assert rows[m, p, i, 1] > 0 and rows[m, p, i, 1] % 256 == 0 and rows[m, p, i, 3] >= rows[m, p, i, 1]
        assert rows[100000, 5, 1, 3] - rows[100000, 5, 1, 1] == 2 * 8 * 100000          # y and o gathered: 8 n each (a multiple of 256)
    g, t = ({tuple(r[:4]): r[4] for r in want[q]} for q in QUERIES)
    assert all(t[c] - g[c] == 8 * 1024 for c in g if c not in REFUSED)


if __name__ == "__main__":
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_dispersion_workspace_cpu.py --record FILE"
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from dlsa_amd import _lib
    with open(sys.argv[2], "w") as f:
        json.dump(record(_lib.load()), f, separators=(",", ":"))
        f.write("\n")
