"""CPU: coverage of the structured ordinal extension header cannot rot.  tests/onehot_ordinal_contract_cases.py is the table of
include/dlsa_hip_onehot_ordinal.h, and this file holds it to what tests/test_ordinal_contract_cpu.py holds the dense family's table
to: every *_workspace_bytes query the extension header declares is named by a case, every function whose last parameter is
`void* stream` is run by a case, and a new entry fails here until it joins."""
import re

import onehot_ordinal_contract_cases as oc


def test_every_declared_query_is_named_by_a_case():
    from dlsa_amd import _lib
    declared = oc.declared_queries()
    # (the parse finds what the binding binds: a declaration the pattern misses would fail here, not pass unnoticed)
    assert declared == sorted(n for n in _lib.ONEHOT_ORDINAL_SIGNATURES if n.endswith("_workspace_bytes")) == [oc.QUERY]
    missing = [q for q in declared if q not in oc.named_queries()]
    assert not missing, "no case of tests/onehot_ordinal_contract_cases.py names %s" % missing
    assert not sorted(oc.named_queries() - set(declared))


def test_every_stream_entry_is_run_by_a_case():
    from dlsa_amd import _lib
    declared = oc.stream_entries()
    assert declared == ["dlsa_onehot_ordinal_pass_f64", "dlsa_onehot_ordinal_fit_f64"]
    for name in declared:                                  # the binding's last argument of each is the stream's void*
        assert _lib.ONEHOT_ORDINAL_SIGNATURES[name][1][-1] is _lib.c_vp, name
    # (nothing the header declares with a trailing stream is missed by the pattern)
    assert len(re.findall(r"void\s*\*\s*stream\s*\)\s*;", oc.header_text())) == len(declared)
    missing = [e for e in declared if e not in oc.named_entries()]
    assert not missing, "no case of tests/onehot_ordinal_contract_cases.py runs %s" % missing
    assert not sorted(oc.named_entries() - set(declared))


def test_a_new_entry_fails_until_it_joins():
    text = oc.header_text() + "\nsize_t dlsa_onehot_ordinal_probit_workspace_bytes(const dlsa_onehot_plan* plan, int64_t n);\n" \
                              "int dlsa_onehot_ordinal_probit_fit_f64(const dlsa_onehot_plan* plan, void* ws, size_t ws_bytes, void* stream);\n"
    assert [q for q in oc.declared_queries(text) if q not in oc.named_queries()] == ["dlsa_onehot_ordinal_probit_workspace_bytes"]
    assert [e for e in oc.stream_entries(text) if e not in oc.named_entries()] == ["dlsa_onehot_ordinal_probit_fit_f64"]


def test_the_table_is_well_formed():
    from dlsa_amd import _lib
    assert len({c.id for c in oc.CASES}) == len(oc.CASES) == 4
    for c in oc.CASES:
        assert c.entries and c.queries and c.refuse == "query" and c.bits, c.id
        assert c.family in ("onehot_ordinal_pass", "onehot_ordinal_fit") and set(c.params) == {"n", "q", "nlevels", "C"}
        for e in c.entries:                                # an entry the extension's table binds, and one that takes a workspace
            assert e in _lib.ONEHOT_ORDINAL_SIGNATURES and _lib.c_sz in _lib.ONEHOT_ORDINAL_SIGNATURES[e][1], (c.id, e)
        # (no entry of the extension hides in the older tables, where their tests would ask for it)
        assert not set(c.entries + c.queries) & (set(_lib.SIGNATURES) | set(_lib.ORDINAL_SIGNATURES))
    assert {(c.params["n"], c.params["q"], c.params["nlevels"], c.params["C"]) for c in oc.CASES} == set(oc.SHAPES)
