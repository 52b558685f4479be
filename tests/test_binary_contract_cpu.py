"""CPU: coverage of the family extension header include/dlsa_hip_binary.h cannot rot.  The frozen contract tables read
include/dlsa_hip.h and _lib.SIGNATURES only; tests/binary_contract_cases.py is the table of this header, and this file holds it to
what tests/test_guarded_workspace_cpu.py and tests/test_stream_contract_cpu.py hold the main tables to: every *_workspace_bytes
query the extension header declares is named by a case, every function whose last parameter is `void* stream` is run by a case, and
a new entry fails here until it joins."""
import re

import binary_contract_cases as bc


def test_every_declared_query_is_named_by_a_case():
    from dlsa_amd import _lib
    declared = bc.declared_queries()
    # (the parse finds what the binding binds: a declaration the pattern misses would fail here, not pass unnoticed)
    assert declared == sorted(n for n in _lib.BINARY_SIGNATURES if n.endswith("_workspace_bytes")) == sorted(bc.QUERIES)
    missing = [q for q in declared if q not in bc.named_queries()]
    assert not missing, "no case of tests/binary_contract_cases.py names %s" % missing
    assert not sorted(bc.named_queries() - set(declared))


def test_every_stream_entry_is_run_by_a_case():
    from dlsa_amd import _lib
    declared = bc.stream_entries()
    assert declared == ["dlsa_probit_pass_f64", "dlsa_probit_fit_f64", "dlsa_cloglog_pass_f64", "dlsa_cloglog_fit_f64"]
    for name in declared:                                  # the binding's last argument of each is the stream's void*
        assert _lib.BINARY_SIGNATURES[name][1][-1] is _lib.c_vp, name
    # (nothing the header declares with a trailing stream is missed by the pattern)
    assert len(re.findall(r"void\s*\*\s*stream\s*\)\s*;", bc.header_text())) == len(declared)
    missing = [e for e in declared if e not in bc.named_entries()]
    assert not missing, "no case of tests/binary_contract_cases.py runs %s" % missing
    assert not sorted(bc.named_entries() - set(declared))


def test_a_new_entry_fails_until_it_joins():
    text = bc.header_text() + "\nsize_t dlsa_cauchit_workspace_bytes(int64_t n, int p);\n" \
                              "int dlsa_cauchit_fit_f64(const double* X, int64_t n, void* ws, size_t ws_bytes, void* stream);\n"
    assert [q for q in bc.declared_queries(text) if q not in bc.named_queries()] == ["dlsa_cauchit_workspace_bytes"]
    assert [e for e in bc.stream_entries(text) if e not in bc.named_entries()] == ["dlsa_cauchit_fit_f64"]


def test_the_table_is_well_formed():
    from dlsa_amd import _lib
    assert len({c.id for c in bc.CASES}) == len(bc.CASES) == 8
    for c in bc.CASES:
        assert c.entries and c.queries and c.refuse == "query" and c.bits, c.id
        assert c.family in ("binary_pass", "binary_fit") and c.params["link"] in bc.LINKS
        for e in c.entries:                                # an entry the extension's table binds, and one that takes a workspace
            assert e in _lib.BINARY_SIGNATURES and _lib.c_sz in _lib.BINARY_SIGNATURES[e][1], (c.id, e)
        # (no entry of the extension hides in another table, where the frozen tests would ask for it)
        assert not set(c.entries + c.queries) & (set(_lib.SIGNATURES) | set(_lib.ORDINAL_SIGNATURES) | set(_lib.ONEHOT_ORDINAL_SIGNATURES))
    assert {c.params["link"] for c in bc.CASES} == set(bc.LINKS)
