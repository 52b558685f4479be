"""The table of the stream-contract test (tests/test_gpu_stream_contract.py), kept where it imports without a GPU and without
torch: tests/test_stream_contract_cpu.py checks against include/dlsa_hip.h that every function whose last parameter is
`void* stream` is named by a selected case of the workspace table, by an extra case below or by an exclusion with its reason, so a
new family fails on the CPU until it joins.

select() keeps every entry tests/workspace_contract_cases.py names and thins duplicates only: all weighted Gram shapes (each a
dispatch class) and one unweighted; for the logistic fits the chains = 1 option set on every shape, plus small = 1 and
batched = 1 on the two shapes that take the one-launch kernel and the lock step; the one-hot families with onehot_ordered = 1, and
with 0 too for onehot_logit_gram; everything else.

EXTRA: the stream-taking entries that bring no workspace and so have no place in that table, each against the check its existing
test applies (the runners are in the GPU test)."""
import collections
import os
import re

import workspace_contract_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LOGISTIC_FITS = ("irls_fit", "irls_fit_ex", "onehot_irls_fit", "onehot_irls_fit_ex")
FORCED_ON = {"K9x2000-p64", "K300x200-p16"}           # where small = 1 / batched = 1 are kept beside chains = 1


def stream_entries(text=None):
    """[name] of every function include/dlsa_hip.h declares with `void* stream` as its last parameter, in header order"""
    if text is None:
        with open(os.path.join(ROOT, "include", "dlsa_hip.h")) as f:
            text = f.read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return [m.group(1) for m in re.finditer(r"\b(dlsa_\w+)\s*\(([^;{}]*?)\)\s*;", text, re.S)
            if re.search(r"\bvoid\s*\*\s*stream\s*$", m.group(2).strip())]


def option_set(case):
    """the name of a logistic-fit case's option set in workspace_contract_cases.OPTION_SETS"""
    for name, opts in wc.OPTION_SETS:
        if case.params.get("options") == opts:
            return name
    raise KeyError(case.id)


def keep(case, unweighted_seen=()):
    """the selection rule for one case of the workspace table; unweighted_seen: the unweighted Gram cases kept so far"""
    if case.family == "gram_f64":
        return bool(case.params["weighted"]) or not unweighted_seen
    if case.family in LOGISTIC_FITS:
        name = option_set(case)
        if name == "chains1":
            return True
        return name in ("small1", "batched1") and any(tag in case.id for tag in FORCED_ON)
    if case.family.startswith("onehot_") and "ordered" in case.params:
        return case.params["ordered"] == 1 or case.family == "onehot_logit_gram"
    return True


def select(cases=None):
    out, unweighted = [], []
    for c in wc.CASES if cases is None else cases:
        if keep(c, unweighted):
            out.append(c)
            if c.family == "gram_f64" and not c.params["weighted"]:
                unweighted.append(c.id)
    return out


SELECTED = select()

# ---- the entries the workspace table cannot name -------------------------------------------------------------------------------
Extra = collections.namedtuple("Extra", "id family entries params bits")
EXTRA = [
    # bit-identical to the oracle on 5000 x 7 rows (tests/test_gpu_kernels.py: test_synth_rows_bit_identical_to_oracle;
    # tests/test_gpu_linear.py: test_synth_response_matches_oracle, test_synth_linear32_matches_oracle_restatement for the bars of
    # the parts that go through transcendental functions)
    Extra("synth_f64-5000-7", "synth", ("dlsa_synth_f64",), dict(n=5000, p=7, dtype="f64"), True),
    Extra("synth_f32-5000-7", "synth", ("dlsa_synth_f32",), dict(n=5000, p=7, dtype="f32"), True),
    Extra("synth_response_f64-5000-7", "synth_response", ("dlsa_synth_f64", "dlsa_synth_response_f64"), dict(n=5000, p=7, dtype="f64"), True),
    Extra("synth_response_f32-5000-7", "synth_response", ("dlsa_synth_f32", "dlsa_synth_response_f32"), dict(n=5000, p=7, dtype="f32"), True),
    Extra("synth_linear_f32-5000-7", "synth_linear32", ("dlsa_synth_linear_f32",), dict(n=5000, p=7), True),
    # the smallest shape of tests/test_gpu_design.py: test_design_kernel_bit_exact, and the smallest with more than one row
    Extra("design-1-1-1-1", "design", ("dlsa_design_f64", "dlsa_design_f32"), dict(n=1, q=1, f=1, p=1), True),
    Extra("design-65-5-0-33", "design", ("dlsa_design_f64", "dlsa_design_f32"), dict(n=65, q=5, f=0, p=33), True),
    Extra("sum_blocks-7-33", "sum_blocks", ("dlsa_sum_blocks_f64",), dict(K=7, p=33), False),
    Extra("negbin_special", "negbin_special", ("dlsa_negbin_special_f64",), dict(), True),
    Extra("sym_pinv_probe-clusters-33", "sym_pinv_probe", ("dlsa_sym_pinv_probe_f64",), dict(kind="clusters", p=33), True),
    # the Python side streams: two chunks of 20 000 x 64, bit for bit the default-stream run
    Extra("fit_linear_streaming-gaussian32", "fit_linear_streaming", ("dlsa_synth_linear_f32", "dlsa_gram_f32_acc64", "dlsa_xtv_stats_f32"),
          dict(rows=20_000, p=64, chunks=2), True),
    Extra("fit_linear_chunks", "fit_linear_chunks", ("dlsa_gram_f32_acc64", "dlsa_xtv_stats_f32"), dict(rows=20_000, p=64, chunks=2), True),
]
assert len({e.id for e in EXTRA}) == len(EXTRA)

# ---- stream-taking entries no case runs, and why --------------------------------------------------------------------------------
_FORWARD = "a one-line forwarder that passes `stream` through to dlsa_cox_%s_strata_f64, which the Cox cases run"
EXCLUDED = {
    "dlsa_cox_pass_f64": _FORWARD % "pass",
    "dlsa_cox_pass_ties_f64": _FORWARD % "pass",
    "dlsa_cox_fit_f64": _FORWARD % "fit",
    "dlsa_cox_fit_ties_f64": _FORWARD % "fit",
    "dlsa_allreduce_f64": "runs on RCCL's own ordering; covered by the distributed tests",
}


def named_entries():
    return {e for c in SELECTED for e in c.entries} | {e for x in EXTRA for e in x.entries}
