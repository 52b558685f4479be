"""The table of the probit / cloglog contract tests (tests/test_gpu_binary_contract.py), kept where it imports without a GPU and
without torch: the entries of the family extension header include/dlsa_hip_binary.h are bound by _lib.BINARY_SIGNATURES, which
the frozen tables of tests/workspace_contract_cases.py and tests/stream_contract_cases.py do not read, so this table holds them to
the same two contracts.  tests/test_binary_contract_cpu.py checks against the extension header that every *_workspace_bytes query
it declares is named by a case and that every function whose last parameter is `void* stream` is run by one.

Cases are workspace_contract_cases.Case tuples, per link: the pass at (2001, 5) without and (2001, 130) with the intercept, the fit
of K = 3 partitions of 1001 rows at p = 5 (contiguous, no intercept) and p = 130 (strided, intercept); offsets everywhere."""
import os
import re

import stream_contract_cases as sc
from workspace_contract_cases import Case

HEADER = os.path.join(sc.ROOT, "include", "dlsa_hip_binary.h")
LINKS = ("probit", "cloglog")
QUERIES = ["dlsa_%s_workspace_bytes" % link for link in LINKS]

CASES = []
for link in LINKS:
    q = "dlsa_%s_workspace_bytes" % link
    for p, icpt, strided in [(5, False, False), (130, True, True)]:
        CASES.append(Case("%s_pass-2001-%d-icpt%d" % (link, p, icpt), "binary_pass", ("dlsa_%s_pass_f64" % link,), (q,), (),
                          dict(link=link, n=2001, p=p, icpt=icpt), True, "query"))
        CASES.append(Case("%s_fit-3x1001-%d-icpt%d-step%s" % (link, p, icpt, "K" if strided else "1"), "binary_fit", ("dlsa_%s_fit_f64" % link,),
                          (q,), (), dict(link=link, rows=1001, K=3, p=p, icpt=icpt, strided=strided), True, "query"))
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
