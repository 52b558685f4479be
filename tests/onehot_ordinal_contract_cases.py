"""The table of the structured ordinal family's contract tests (tests/test_gpu_onehot_ordinal_contract.py), kept where it imports
without a GPU: the entries of the family extension header include/dlsa_hip_onehot_ordinal.h are bound by
_lib.ONEHOT_ORDINAL_SIGNATURES, which neither the frozen tables of tests/workspace_contract_cases.py and
tests/stream_contract_cases.py nor tests/ordinal_contract_cases.py read, so this table holds them to the same two contracts.
tests/test_onehot_ordinal_contract_cpu.py checks against the extension header that every *_workspace_bytes query it declares is
named by a case and that every function whose last parameter is `void* stream` is run by one.

Cases are workspace_contract_cases.Case tuples: pass and fit at (6001, 2, (5, 4), C = 3) and (6001, 3, (40, 9), C = 8), baselines
dropped, no constant column (p = 9 and p = 50, d = 11 and d = 57; 8 classes carry the in-pass borders of all seven cutpoints)."""
import os
import re

import stream_contract_cases as sc
from workspace_contract_cases import Case

HEADER = os.path.join(sc.ROOT, "include", "dlsa_hip_onehot_ordinal.h")
QUERY = "dlsa_onehot_ordinal_workspace_bytes"
SHAPES = [(6001, 2, (5, 4), 3), (6001, 3, (40, 9), 8)]

CASES = []
for n, q, nlevels, C in SHAPES:
    for kind in ("pass", "fit"):
        CASES.append(Case("onehot_ordinal_%s-%d-%d-%s-C%d" % (kind, n, q, "x".join(map(str, nlevels)), C), "onehot_ordinal_" + kind,
                          ("dlsa_onehot_ordinal_%s_f64" % kind,), (QUERY,), (), dict(n=n, q=q, nlevels=nlevels, C=C), True, "query"))
assert len({c.id for c in CASES}) == len(CASES)


def header_text():
    with open(HEADER) as f:
        return f.read()


def declared_queries(text=None):
    """every *_workspace_bytes query the extension header declares"""
    text = re.sub(r"/\*.*?\*/", " ", header_text() if text is None else text, flags=re.S)
    return sorted(set(re.findall(r"^\s*size_t\s+(dlsa_\w+_workspace_bytes)\s*\(", text, re.M)))


def stream_entries(text=None):
    """every function the extension header declares with `void* stream` as its last parameter (the parse of the main table)"""
    return sc.stream_entries(header_text() if text is None else text)


def named_queries():
    return {q for c in CASES for q in c.queries + c.also}


def named_entries():
    return {e for c in CASES for e in c.entries}
