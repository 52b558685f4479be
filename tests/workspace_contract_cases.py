"""The table of the workspace-contract test (tests/test_gpu_workspace_contract.py), kept where it imports without a GPU and
without torch: tests/test_guarded_workspace_cpu.py checks against include/dlsa_hip.h that every dlsa_*_workspace_bytes query
the header declares is named by at least one case, so a new family fails on the CPU until it joins the table.

A case names the runner that makes its engine calls (`family`), the C entry points it must reach (`entries`), the queries
the engine sizes the scratch with (`queries`: checked at run time against the calls the library saw), further queries the
runner pins to those (`also`: the Cox queries the header declares equal for the unstratified model) and the runner's
parameters.  `bits`: the entry's existing test asserts bit-reproducibility, so the 0xFF-body run must equal a 0x00-body run
bit for bit.  `refuse`: how the refusals are taken -- "query" (ws_bytes = query - 1 and the pointer offset by 8), or
"chains1" (the logistic fits accept one chain's slice: both under irls_options(chains=1), where the query is one slice), or
"need" (the three Gram entries, the two loglik entries and xtv_f32 check the need of the kernel the shape dispatches, which is
at most the query: that need, taken from the message of a 256-byte call, minus 1 -- csrc/gram.hip and csrc/logit.hip are
pinned by the source hashes of the committed counter profiles, so these entries were left as they are)."""
import collections

Case = collections.namedtuple("Case", "id family entries queries also params bits refuse")

CASES = []


def case(id, family, entries, queries, params, also=(), bits=False, refuse="query"):
    entries = (entries,) if isinstance(entries, str) else tuple(entries)
    queries = (queries,) if isinstance(queries, str) else tuple(queries)
    CASES.append(Case(id, family, entries, queries, tuple(also), dict(params), bits, refuse))


GRAM = "dlsa_gram_workspace_bytes"
LOGIT = "dlsa_logit_workspace_bytes"

# ---- Gram: one (n, p) per dispatch class of dlsa_gram_f64, weighted and unweighted; two padded row pitches ------------------
GRAM_SHAPES = [(33, 2), (8193, 50), (20011, 120), (9001, 125), (5003, 260), (4001, 500), (3001, 572), (2001, 600)]
for n, p in GRAM_SHAPES:
    for weighted in (True, False):
        case("gram_f64-%d-%d-%s" % (n, p, "w" if weighted else "1"), "gram_f64", "dlsa_gram_f64", GRAM, dict(n=n, p=p, weighted=weighted, ld=p),
             refuse="need")
case("gram_f64-33-2-w-ld6", "gram_f64", "dlsa_gram_f64", GRAM, dict(n=33, p=2, weighted=True, ld=6), refuse="need")
case("gram_f64-5003-260-w-ld263", "gram_f64", "dlsa_gram_f64", GRAM, dict(n=5003, p=260, weighted=True, ld=263), refuse="need")
# (beyond the list above, whose 125 .. 600 column shapes all run on the panel kernel: the plan kernel needs 32768 rows -- 8 tiles on
#  one CU, 19 on a two-CU group with its pacing counts in the workspace -- and the cyclic kernel 65536 rows at 481 .. 508 columns)
for n, p in [(32771, 125), (32771, 300), (65537, 500)]:
    case("gram_f64-%d-%d-w" % (n, p), "gram_f64", "dlsa_gram_f64", GRAM, dict(n=n, p=p, weighted=True, ld=p + (p & 1)), refuse="need")
case("gram_f64-32771-300-1", "gram_f64", "dlsa_gram_f64", GRAM, dict(n=32771, p=300, weighted=False, ld=300), refuse="need")
for n, p in [(16384, 768), (777, 100)]:
    case("gram_f32-%d-%d" % (n, p), "gram_f32", "dlsa_gram_f32", GRAM, dict(n=n, p=p), refuse="need")
    case("gram_f32_acc64-%d-%d" % (n, p), "gram_f32_acc64", "dlsa_gram_f32_acc64", GRAM, dict(n=n, p=p), refuse="need")

# ---- X'v ------------------------------------------------------------------------------------------------------------------
case("xtv_f64-4099-129", "xtv", "dlsa_xtv_f64", LOGIT, dict(n=4099, p=129, dtype="f64"))
case("xtv_f32-20001-300", "xtv", "dlsa_xtv_f32", LOGIT, dict(n=20001, p=300, dtype="f32"), refuse="need")          # the engine passes twice the query
for dtype, n, p in [("f64", 5001, 37), ("f32", 5001, 37), ("f32", 20001, 999)]:
    case("xtv_stats_%s-%d-%d" % (dtype, n, p), "xtv_stats", "dlsa_xtv_stats_" + dtype, "dlsa_xtv_stats_workspace_bytes",
         dict(n=n, p=p, dtype=dtype), bits=True)

# ---- the logit passes ------------------------------------------------------------------------------------------------------
for p in (2, 50, 121, 500):
    for icpt in (False, True):
        sfx = "_icpt" if icpt else ""
        case("logit_pass%s-%d" % (sfx, p), "logit_pass", "dlsa_logit_pass%s_f64" % sfx, LOGIT, dict(n=4099, p=p, icpt=icpt))
        case("loglik%s-%d" % (sfx, p), "loglik", "dlsa_loglik%s_f64" % sfx, LOGIT, dict(n=4099, p=p, icpt=icpt, cols=3), refuse="need")
case("irls_pass-8192-50-fused", "irls_pass", "dlsa_irls_pass_f64", "dlsa_irls_pass_workspace_bytes", dict(n=8192, p=50, fused=True), bits=True)
case("irls_pass-8191-51-two-launch", "irls_pass", "dlsa_irls_pass_f64", "dlsa_irls_pass_workspace_bytes", dict(n=8191, p=51, fused=False))
for p, icpt in [(121, False), (200, True)]:
    case("newton_wide_pass-32785-%d-%d" % (p, icpt), "newton_wide_pass", ("dlsa_newton_wide_pass_f64", "dlsa_logit_pass%s_f64" % ("_icpt" if icpt else "")),
         ("dlsa_newton_wide_workspace_bytes", LOGIT), dict(n=32785, p=p, icpt=icpt), bits=True)
for p in (120, 500):
    case("gram_icpt-5001-%d" % p, "gram_icpt", ("dlsa_gram_icpt_f64", "dlsa_logit_pass_icpt_f64", "dlsa_loglik_icpt_f64"),
         ("dlsa_gram_icpt_workspace_bytes", LOGIT), dict(n=5001, p=p))

# ---- the logistic fits: at the query under default options, under chains = 1, and with small / batched forced on and off ------
# (K = 9 x 2000 at p = 64 is not in the list the fits were given: it is the one shape here whose width the lock step serves, so that
#  batched = 1 shows driver 2, whose memory comes from the stream's pool and not from ws)
IRLS_SHAPES = [dict(tag="K9x2000-p8", K=9, rows=2000, p=8), dict(tag="K9x2000-p64", K=9, rows=2000, p=64), dict(tag="K300x200-p16", K=300, rows=200, p=16),
               dict(tag="K3x70001-p40", K=3, rows=70001, p=40), dict(tag="K2x33000-p120", K=2, rows=33000, p=120),
               dict(tag="K2x40000-p200", K=2, rows=40000, p=200)]
OPTION_SETS = [("default", {}), ("chains1", dict(chains=1)), ("small1", dict(small=True)), ("small0", dict(small=False)),
               ("batched1", dict(batched=True)), ("batched0", dict(batched=False))]


def _irls_cases():
    for s in IRLS_SHAPES:
        wide = s["p"] >= 120
        for oname, opts in OPTION_SETS:
            # (forcing the one-launch kernel / the lock step is only defined where the shape is eligible: the many-partition shapes)
            if oname in ("small1", "batched1") and s["K"] < 9:
                continue
            if wide and oname in ("small0", "batched0"):
                continue
            base = dict(K=s["K"], rows=s["rows"], p=s["p"], options=opts)
            if not wide:
                case("irls_fit-%s-%s" % (s["tag"], oname), "irls_fit", "dlsa_irls_fit_f64", "dlsa_irls_workspace_bytes", base,
                     bits=True, refuse="chains1")
                case("irls_fit_ex-%s-icpt-step-%s" % (s["tag"], oname), "irls_fit_ex", "dlsa_irls_fit_ex_f64", "dlsa_irls_ex_workspace_bytes",
                     dict(base, icpt=True, strided=True), bits=True, refuse="chains1")
            elif s["p"] == 120:
                case("irls_fit_ex-%s-icpt-%s" % (s["tag"], oname), "irls_fit_ex", "dlsa_irls_fit_ex_f64", "dlsa_irls_ex_workspace_bytes",
                     dict(base, icpt=True, strided=False), bits=True, refuse="chains1")
            else:
                case("irls_fit-%s-%s" % (s["tag"], oname), "irls_fit", "dlsa_irls_fit_f64", "dlsa_irls_workspace_bytes", base,
                     bits=True, refuse="chains1")
                for icpt in (False, True):
                    for strided in (False, True):
                        case("irls_fit_ex-%s-icpt%d-step%s-%s" % (s["tag"], icpt, "K" if strided else "1", oname), "irls_fit_ex",
                             "dlsa_irls_fit_ex_f64", "dlsa_irls_ex_workspace_bytes", dict(base, icpt=icpt, strided=strided), bits=True,
                             refuse="chains1")


_irls_cases()
for oname, opts in OPTION_SETS:
    case("onehot_irls_fit-%s" % oname, "onehot_irls_fit", "dlsa_onehot_irls_fit_f64", "dlsa_onehot_irls_workspace_bytes",
         dict(n=30000, q=4, nlevels=(9, 5, 30), options=opts), bits=True, refuse="chains1")
    case("onehot_irls_fit_ex-%s" % oname, "onehot_irls_fit_ex", "dlsa_onehot_irls_fit_ex_f64", "dlsa_onehot_irls_ex_workspace_bytes",
         dict(n=30001, q=3, nlevels=(7, 4, 12), K=3, options=opts), bits=True, refuse="chains1")

# ---- Cox: Breslow, Efron, Efron with strata; tied times -------------------------------------------------------------------
COX = "dlsa_cox_strata_workspace_bytes"
COX_ALSO = ("dlsa_cox_workspace_bytes", "dlsa_cox_ties_workspace_bytes")      # equal to the strata query of the unstratified model
for ties, strata in [("breslow", False), ("efron", False), ("efron", True)]:
    tag = ties + ("-strata" if strata else "")
    for p in (7, 130):
        case("cox_pass-%s-5003-%d" % (tag, p), "cox_pass", "dlsa_cox_pass_strata_f64", COX, dict(n=5003, p=p, ties=ties, strata=strata),
             also=() if strata else COX_ALSO)
        case("cox_fit-%s-5003-%d" % (tag, p), "cox_fit", "dlsa_cox_fit_strata_f64", COX, dict(n=5003, p=p, ties=ties, strata=strata, K=3),
             also=() if strata else COX_ALSO, bits=True)

# ---- the count families: pass and fit, p = 5 and 130, intercept 0 and 1, with offset; fits with row_step 1 and K = 3 -------
for fam in ("poisson", "negbin", "gamma", "tweedie"):
    q = "dlsa_%s_workspace_bytes" % fam
    for p in (5, 130):
        for icpt in (False, True):
            case("%s_pass-4001-%d-icpt%d" % (fam, p, icpt), fam + "_pass", "dlsa_%s_pass_f64" % fam, q, dict(n=4001, p=p, icpt=icpt), bits=True)
            for strided in (False, True):
                case("%s_fit-3x4001-%d-icpt%d-step%s" % (fam, p, icpt, "K" if strided else "1"), fam + "_fit", "dlsa_%s_fit_f64" % fam, q,
                     dict(rows=4001, K=3, p=p, icpt=icpt, strided=strided), bits=True)

# ---- multinomial: classes 2, 3 and 8 at p = 5 with intercept; p = 40 with 8 classes (J pe = 287: the plan class) --------------
for C, p in [(2, 5), (3, 5), (8, 5), (8, 40)]:
    case("multinomial_pass-6001-%d-C%d" % (p, C), "multinomial_pass", "dlsa_multinomial_pass_f64", "dlsa_multinomial_workspace_bytes",
         dict(n=6001, p=p, C=C, icpt=True), bits=True)
    case("multinomial_fit-6001-%d-C%d" % (p, C), "multinomial_fit", "dlsa_multinomial_fit_f64", "dlsa_multinomial_workspace_bytes",
         dict(n=6001, p=p, C=C, icpt=True), bits=True)

# ---- the structured one-hot families: the plans and smallest sizes of their own test files, onehot_ordered 0 and 1 -----------
ONEHOT_PLANS = [dict(n=257, q=0, nlevels=(3, 2), intercept=False, baseline=False), dict(n=777, q=7, nlevels=(40, 40, 9, 2), intercept=True, baseline=True)]
for ordered in (1, 0):
    for pl in ONEHOT_PLANS:
        tag = "%d-%d-%s-ord%d" % (pl["n"], pl["q"], "x".join(map(str, pl["nlevels"])), ordered)
        case("onehot_logit_gram-" + tag, "onehot_logit_gram", ("dlsa_onehot_logit_pass_f64", "dlsa_onehot_gram_f64"), "dlsa_onehot_workspace_bytes",
             dict(pl, ordered=ordered), bits=bool(ordered))
        for fam in ("poisson", "negbin", "gamma", "tweedie", "multinomial"):
            case("onehot_%s_pass-%s" % (fam, tag), "onehot_%s_pass" % fam, "dlsa_onehot_%s_pass_f64" % fam, "dlsa_onehot_%s_workspace_bytes" % fam,
                 dict(pl, ordered=ordered), bits=bool(ordered))
    for fam in ("poisson", "negbin", "gamma", "tweedie", "multinomial"):
        case("onehot_%s_fit-ord%d" % (fam, ordered), "onehot_%s_fit" % fam, "dlsa_onehot_%s_fit_f64" % fam, "dlsa_onehot_%s_workspace_bytes" % fam,
             dict(ordered=ordered), bits=bool(ordered))

# ---- the solvers ----------------------------------------------------------------------------------------------------------
for p in (1, 112, 113, 500):
    case("spd_solve-%d" % p, "spd_solve", "dlsa_spd_solve_f64", "dlsa_solve_workspace_bytes", dict(p=p))
for p in (3, 260):
    case("wls_solve-%d" % p, "wls_solve", "dlsa_wls_solve_f64", "dlsa_wls_solve_workspace_bytes", dict(p=p))
    case("sym_pinv_solve-%d" % p, "sym_pinv_solve", "dlsa_sym_pinv_solve_f64", "dlsa_sym_pinv_workspace_bytes", dict(p=p))
for route in ("factor", "reuse", "inverse", "sweep"):
    for p in (112, 113):
        if route == "sweep" and p > 112:
            continue                                                  # (the sweep's registers hold 112: 113 is refused as invalid)
        case("newton_solve_probe-%s-%d" % (route, p), "newton_probe", "dlsa_newton_solve_probe_f64", "dlsa_newton_solve_probe_workspace_bytes",
             dict(route=route, p=p))
case("newton_solve_probe-sweep_batched-112-count5", "newton_probe_batched", "dlsa_newton_solve_probe_f64", "dlsa_newton_solve_probe_workspace_bytes",
     dict(p=112))
case("newton_solve_probe-sweep_batched-112-count1", "newton_probe_batched1", "dlsa_newton_solve_probe_f64", "dlsa_newton_solve_probe_workspace_bytes",
     dict(p=112))

# ---- LARS: lars_q.hip, lars.hip (lars_q = 0) and lars_c.hip (by default beyond 448 variables; lars_q = 2 from 64) ------------
for p, kopt in [(3, {}), (120, {}), (120, dict(lars_q=0)), (120, dict(lars_q=2)), (257, {}), (257, dict(lars_q=0)), (257, dict(lars_q=2)),
                (1030, {}), (1030, dict(lars_q=0))]:
    case("lars_lsa-%d%s" % (p, "".join("-%s%d" % kv for kv in kopt.items())), "lars", "dlsa_lars_lsa_f64", "dlsa_lars_workspace_bytes",
         dict(p=p, kopt=kopt), bits=(p == 1030 and not kopt))

assert len({c.id for c in CASES}) == len(CASES)
