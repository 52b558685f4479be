"""CPU: the stream-contract test (tests/test_gpu_stream_contract.py) cannot lose an entry point without this file noticing -- every
function of include/dlsa_hip.h whose last parameter is `void* stream` is named by a selected case, an extra case or an exclusion
with a reason -- and its tools that need no GPU (the selection rule, PoisonTorch) do what they say."""
import pytest

import stream_contract_cases as sc
import workspace_contract_cases as wc

torch = pytest.importorskip("torch")


# ---- coverage cannot rot ------------------------------------------------------------------------------------------------------
def test_the_header_parse_finds_what_the_binding_binds():
    from dlsa_amd import _lib
    declared = sc.stream_entries()
    assert len(declared) == len(set(declared)) >= 62, len(declared)
    for name in declared:                                  # the binding's last argument of each is the stream's void*
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][1][-1] is _lib.c_vp, name
    # (and nothing the binding binds with a trailing stream is missed by the pattern: a declaration it cannot read fails here)
    text = open(sc.os.path.join(sc.ROOT, "include", "dlsa_hip.h")).read()
    assert len(sc.re.findall(r"void\s*\*\s*stream\s*\)\s*;", text)) == len(declared)


def test_the_parse_reads_only_a_trailing_stream():
    text = """
    int dlsa_a_f64(const double* X, int64_t n,
                   void* ws, size_t ws_bytes, void* stream);
    /* int dlsa_commented_f64(void* stream); */
    int dlsa_b(void* stream, int n);
    size_t dlsa_b_workspace_bytes(int p);
    int dlsa_c_f32(void *stream);      // int dlsa_d(void* stream);
    """
    assert sc.stream_entries(text) == ["dlsa_a_f64", "dlsa_c_f32"]


def test_every_stream_entry_is_named_or_excluded_with_a_reason():
    declared = sc.stream_entries()
    named = sc.named_entries()
    assert not sorted(named - set(declared)), sorted(named - set(declared))
    assert not sorted(set(sc.EXCLUDED) - set(declared)), "an exclusion names no declared entry"
    assert not sorted(set(sc.EXCLUDED) & named), "an excluded entry is run after all: drop the exclusion"
    missing = [e for e in declared if e not in named and e not in sc.EXCLUDED]
    assert not missing, "no case of the stream-contract test runs %s: add a case (tests/workspace_contract_cases.py, or EXTRA in " \
                        "tests/stream_contract_cases.py) or an exclusion with its reason" % missing
    assert sorted(sc.EXCLUDED) == ["dlsa_allreduce_f64", "dlsa_cox_fit_f64", "dlsa_cox_fit_ties_f64", "dlsa_cox_pass_f64", "dlsa_cox_pass_ties_f64"]
    assert all(len(reason) > 20 for reason in sc.EXCLUDED.values())


def test_a_new_family_fails_until_it_joins():
    """the check of the test above on a header with one more stream-taking entry"""
    with open(sc.os.path.join(sc.ROOT, "include", "dlsa_hip.h")) as f:
        text = f.read() + "\nint dlsa_probit_fit_f64(const double* X, int64_t n, void* ws, size_t ws_bytes, void* stream);\n"
    named = sc.named_entries()
    assert [e for e in sc.stream_entries(text) if e not in named and e not in sc.EXCLUDED] == ["dlsa_probit_fit_f64"]


# ---- the selection rule ---------------------------------------------------------------------------------------------------------
def test_selection_keeps_every_entry_and_thins_only_duplicates():
    all_entries = {e for c in wc.CASES for e in c.entries}
    assert {e for c in sc.SELECTED for e in c.entries} == all_entries
    ids = {c.id for c in sc.SELECTED}
    assert len(ids) == len(sc.SELECTED) < len(wc.CASES)
    by_family = lambda cases, fam: [c for c in cases if c.family == fam]
    # Gram: every weighted shape, one unweighted
    g_all, g_sel = by_family(wc.CASES, "gram_f64"), by_family(sc.SELECTED, "gram_f64")
    assert [c.id for c in g_sel if c.params["weighted"]] == [c.id for c in g_all if c.params["weighted"]]
    assert len([c for c in g_sel if not c.params["weighted"]]) == 1
    # the logistic fits: chains = 1 on every shape, small = 1 / batched = 1 on two
    for fam in sc.LOGISTIC_FITS:
        sel = by_family(sc.SELECTED, fam)
        assert [c.id for c in sel if sc.option_set(c) == "chains1"] == [c.id for c in by_family(wc.CASES, fam) if sc.option_set(c) == "chains1"]
        forced = [c for c in sel if sc.option_set(c) != "chains1"]
        assert all(sc.option_set(c) in ("small1", "batched1") and any(t in c.id for t in sc.FORCED_ON) for c in forced)
        if fam in ("irls_fit", "irls_fit_ex"):
            assert {(sc.option_set(c), t) for c in forced for t in sc.FORCED_ON if t in c.id} == {(o, t) for o in ("small1", "batched1") for t in sc.FORCED_ON}
    shapes = {(c.params["K"], c.params["rows"], c.params["p"]) for c in sc.SELECTED if c.family in ("irls_fit", "irls_fit_ex")}
    assert shapes == {(s["K"], s["rows"], s["p"]) for s in wc.IRLS_SHAPES}
    # one-hot: ordered = 1, and 0 as well for onehot_logit_gram
    for c in wc.CASES:
        if c.family.startswith("onehot_") and "ordered" in c.params:
            assert (c.id in ids) == (c.params["ordered"] == 1 or c.family == "onehot_logit_gram"), c.id
    # every other family: everything
    thinned = {"gram_f64"} | set(sc.LOGISTIC_FITS) | {c.family for c in wc.CASES if c.family.startswith("onehot_") and "ordered" in c.params}
    assert all(c.id in ids for c in wc.CASES if c.family not in thinned)
    print("stream contract: %d selected cases of %d, %d extra" % (len(sc.SELECTED), len(wc.CASES), len(sc.EXTRA)))


def test_extra_cases_are_well_formed():
    from dlsa_amd import _lib
    table = {e for c in wc.CASES for e in c.entries}
    for x in sc.EXTRA:
        assert x.entries and all(e in _lib.SIGNATURES for e in x.entries), x.id
    # an extra case is there for entries the workspace table cannot name
    assert all(any(e not in table for e in x.entries) or x.family.startswith("fit_linear") for x in sc.EXTRA)


# ---- PoisonTorch on CPU tensors ---------------------------------------------------------------------------------------------------
def test_poison_torch_fills_empty_and_leaves_zeros():
    import stream_gate as sg
    pt = sg.PoisonTorch()
    f = pt.empty((3, 5), dtype=torch.float64)
    h = pt.empty(7, dtype=torch.float32)
    i = pt.empty((4,), dtype=torch.int32)
    b = pt.empty((6,), dtype=torch.uint8)
    assert bool(torch.isnan(f).all()) and bool(torch.isnan(h).all()) and f.shape == (3, 5) and f.dtype == torch.float64
    assert bool((i == 77).all()) and bool((b == 77).all()) and i.dtype == torch.int32
    assert pt.empty((0, 4), dtype=torch.float64).numel() == 0 and pt.empty((), dtype=torch.float64).element_size() == 8
    z = pt.zeros((2, 2), dtype=torch.float64)
    assert bool((z == 0).all()) and bool((pt.zeros(3, dtype=torch.int64) == 0).all())
    # everything else is torch's own
    assert pt.float64 is torch.float64 and pt.is_tensor(f) and pt.cuda is torch.cuda and pt.from_numpy is torch.from_numpy
    assert pt.made == 6


def test_poison_torch_stands_in_for_the_engines_torch(monkeypatch):
    import stream_gate as sg
    from dlsa_amd import engine
    monkeypatch.setattr(engine, "torch", sg.PoisonTorch())
    X = engine.empty_rows(4, 3, torch.float64, "cpu")                  # an odd fp64 width: one pad element per row, zeroed by the engine
    assert X.shape == (4, 3) and X.stride(0) == 4 and bool(torch.isnan(X).all())
    with pytest.raises(RuntimeError, match="GPU only"):                # the wrappers' own checks still run
        engine.gram(X)


def test_the_gate_is_bounded():
    import stream_gate as sg
    assert 0 < sg.MAX_GATE_SECONDS <= 3.0 and sg.CANDIDATES == 8
