"""The table of the ordinal family's contract tests (tests/test_gpu_ordinal_contract.py), kept where it imports without a GPU and
without torch: the entries of the family extension header include/dlsa_hip_ordinal.h are bound by _lib.ORDINAL_SIGNATURES, which
the frozen tables of tests/workspace_contract_cases.py and tests/stream_contract_cases.py do not read, so this table holds them to
the same two contracts.  tests/test_ordinal_contract_cpu.py checks against the extension header that every *_workspace_bytes query
it declares is named by a case and that every function whose last parameter is `void* stream` is run by one.

Cases are workspace_contract_cases.Case tuples: pass and fit at (6001, 5, 3) and (6001, 40, 8), the shapes of the multinomial
cases (d = 7 and d = 47; 8 classes carry the in-pass borders of all seven cutpoints)."""
import os
import re

import stream_contract_cases as sc
from workspace_contract_cases import Case

HEADER = os.path.join(sc.ROOT, "include", "dlsa_hip_ordinal.h")
QUERY = "dlsa_ordinal_workspace_bytes"

CASES = []
for n, p, C in [(6001, 5, 3), (6001, 40, 8)]:
    for kind in ("pass", "fit"):
        CASES.append(Case("ordinal_%s-%d-%d-C%d" % (kind, n, p, C), "ordinal_" + kind, ("dlsa_ordinal_%s_f64" % kind,), (QUERY,), (),
                          dict(n=n, p=p, C=C), True, "query"))
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
