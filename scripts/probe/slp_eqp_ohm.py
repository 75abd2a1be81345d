"""SLP-EQP with the exact Hessian of the Ohm's-law block (nlp_kind 4: acopf.function_model(case, hessian=True); DESIGN.md "Second
derivatives of the Ohm's-law block") beside the two ways the same model ran SLP-EQP before: the limited-memory Hessian on the Ohm's-law
kernel (nlp_kind 1) and the exact Hessian of the expression form (nlp="expr").

  runs      (default) the case118-sized ACOPF: SLP-EQP exact on kind 4, SLP-EQP limited-memory on kind 1, SLP-EQP exact on expressions,
            each whole inside the library on a fresh handle (set-up outside the clock; the clock is the host's around one C call that ends
            with its results on the host).  One warm-up run of each, then --reps (default 5) rounds in ABCCBA order: 10 timed runs each.
  hessians  --hessians case118,case1354pegase: asm_eval_hessian_lagrangian alone, for a kernel trace taken in a run of its own
            (k_nlp_ohm_hess + k_nlp_expr_hess_gather on kind 4 against k_nlp_expr_hess + k_nlp_expr_hess_gather on expressions).  Per
            case and model --reps calls after a warm-up; the host times it prints hold the whole call, copies included.
  batch     --batch S (e.g. 64): asm_batch_slp_run_eqp on S load scenarios of the case118-sized ACOPF, kind 4 against expressions (the
            batch of scripts/probe/batch_eqp.py), a batch of S slots each, one warm-up and --reps (default 3) rounds in ABBA order.

Prints one JSON line per case; --out FILE appends them there; --load S (default 1.0 for case118, 0.5 otherwise); --max-iter K (default
200); --tr-size D (default 0.4); --memory P (default 10)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import acopf, batch  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def handle(fm, pr):
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    return opt


def one_run(fm, pr, par):
    opt = handle(fm, pr)
    if par.hessian_type == "limited-memory":
        opt.set_hessian_type("limited-memory", par.lm_memory)
    t0 = time.perf_counter()
    run = opt.slp_run(pr.x0, par)
    ms = 1e3 * (time.perf_counter() - t0)
    opt.close()
    return ms, run


def emit(out):
    line = json.dumps(out)
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write(line + "\n")


def spread(ms):
    return dict(ms_median=float(np.median(ms)), ms_min=float(min(ms)), ms_max=float(max(ms)))


def runs(case):
    reps, max_iter, tr_size, memory = arg("--reps", 5), arg("--max-iter", 200), arg("--tr-size", 0.4), arg("--memory", 10)
    load = arg("--load", 1.0 if case == "case118" else 0.5)
    grid = acopf.synthetic_case(case, 1, load)
    kw = dict(max_iter=max_iter, tr_size=tr_size, device_eval=True)
    setups = {"eqp_ohm_hess": (acopf.function_model(grid, hessian=True), A.Parameters(algorithm="SLP-EQP", **kw)),
              "eqp_lm": (acopf.function_model(grid), A.Parameters(algorithm="SLP-EQP", hessian_type="limited-memory", lm_memory=memory, **kw)),
              "eqp_expr": (acopf.function_model(grid, nlp="expr"), A.Parameters(algorithm="SLP-EQP", **kw))}
    prs = {k: fm.to_problem("%s-sized" % case) for k, (fm, _) in setups.items()}
    ms, last = {k: [] for k in setups}, {}
    for k, (fm, par) in setups.items():              # code objects, pinned staging: not part of any timing
        one_run(fm, prs[k], par)
    order = list(setups) + list(setups)[::-1]
    for _ in range(reps):
        for k in order:
            t, last[k] = one_run(setups[k][0], prs[k], setups[k][1])
            ms[k].append(t)
    out = dict(mode="runs", case=case, load=load, n=int(prs["eqp_lm"].n), m=int(prs["eqp_lm"].m), max_iter=max_iter, tr_size=tr_size, memory=memory, reps=2 * reps)
    for k, r in last.items():
        out[k] = dict(status=r.ret, iter=r.iter, lp_solves=r.lp_solves, restoration_solves=r.restoration_solves, obj_val=r.obj_val, prim_infeas=r.prim_infeas,
                      dual_infeas=r.dual_infeas, compl=r.compl, counts=r.eqp_counts, radius=r.Delta_E, **spread(ms[k]))
    emit(out)


def hessians(case):
    reps = arg("--reps", 5)
    grid = acopf.synthetic_case(case, 1, arg("--load", 1.0 if case == "case118" else 0.5))
    out = dict(mode="hessians", case=case, reps=reps)
    rng = np.random.default_rng(1)
    for key, fm in (("ohm_hess", acopf.function_model(grid, hessian=True)), ("expr", acopf.function_model(grid, nlp="expr"))):
        pr = fm.to_problem(case)
        opt = handle(fm, pr)
        x, lam = pr.x0 + 0.01 * rng.standard_normal(pr.n), rng.standard_normal(pr.m)
        nnz = len(opt.eval_hessian_lagrangian(x, 1.0, lam))
        t = []
        for _ in range(reps):
            t0 = time.perf_counter()
            opt.eval_hessian_lagrangian(x, 1.0, lam)
            t.append(1e3 * (time.perf_counter() - t0))
        out[key] = dict(n=int(pr.n), m=int(pr.m), nnz=nnz, branches=int(fm.acopf_model.nl), **spread(t))
        opt.close()
    emit(out)


def batches(S):
    reps, max_iter = arg("--reps", 3), arg("--max-iter", 200)
    case, load = "case118", arg("--load", 1.0)
    base = acopf.synthetic_case(case, 1, load)
    par = A.Parameters(algorithm="SLP-EQP", max_iter=max_iter, device_eval=True)
    models = {"ohm_hess": lambda c: acopf.function_model(c, hessian=True), "expr": lambda c: acopf.function_model(c, nlp="expr")}
    prs = {k: [mk(acopf.scenario_case(base, s)).to_problem("%s-sized scenario %d" % (case, s)) for s in range(S)] for k, mk in models.items()}
    stacks = {k: tuple(np.stack([getattr(p, f) for p in v]) for f in ("g_L", "g_U", "x_L", "x_U", "x0")) for k, v in prs.items()}
    hbs = {k: batch.HipBatch(v[0], S) for k, v in prs.items()}

    def run(k):
        t0 = time.perf_counter()
        got = hbs[k].slp_run(*stacks[k], par)
        ms = 1e3 * (time.perf_counter() - t0)
        print("[slp_eqp_ohm] batch S=%d %s: %.0f ms" % (S, k, ms), file=sys.stderr, flush=True)
        return ms, got
    ms, last = {k: [] for k in hbs}, {}
    for k in hbs:
        run(k)
    for _ in range(reps):
        for k in ("ohm_hess", "expr", "expr", "ohm_hess"):
            t, last[k] = run(k)
            ms[k].append(t)
    out = dict(mode="batch", case=case, load=load, scenarios=S, n=int(prs["expr"][0].n), m=int(prs["expr"][0].m), max_iter=max_iter, reps=2 * reps)
    for k, rs in last.items():
        out[k] = dict(converged=sum(1 for r in rs if r.ret == 0), iterations=sum(r.iter for r in rs), lp_solves=sum(r.lp_solves for r in rs),
                      eqp_counts={c: sum(r.eqp_counts[c] for r in rs) for c in rs[0].eqp_counts}, **spread(ms[k]))
        hbs[k].close()
    emit(out)


def main():
    if "--hessians" in sys.argv:
        for case in arg("--hessians", "").split(","):
            hessians(case)
    elif "--batch" in sys.argv:
        batches(arg("--batch", 64))
    else:
        for case in arg("--cases", "case118").split(","):
            runs(case)


if __name__ == "__main__":
    main()
