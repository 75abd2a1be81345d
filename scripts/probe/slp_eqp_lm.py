"""SLP-EQP with the limited-memory Hessian (asm_hessian_set_type, DESIGN.md "Limited-memory Hessian") on the Ohm's-law ACOPF, which has
no second derivatives, beside the Trust-Region SLP on the same model and SLP-EQP with the exact Hessian on the expression form.

  runs      (default) the case118-sized ACOPF: Trust Region (Ohm's-law kernel), SLP-EQP limited-memory (Ohm's-law kernel), SLP-EQP exact
            (expressions), each whole inside the library on a fresh handle (set-up outside the clock; the clock is the host's around one C
            call that ends with its results on the host).  One warm-up run of each, then --reps (default 5) rounds in ABCCBA order.
  products  --products case118,case1354pegase: the Hessian products alone, for a kernel trace.  Per case a handle on the Ohm's-law model
            with --memory (default 10) stored pairs and a handle on the expression model; on each, asm_kkt_step (one-column products) and
            asm_kkt_step_multi with 64 columns on the empty working set (no factor: the calls are products and reductions), --reps times
            after a warm-up.  The host times it prints hold the whole call; the time of k_lm_psi_v, k_lm_apply, k_hess_product and
            k_kktm_hess_product<64> comes from a kernel trace of this mode, taken in a run of its own.

Prints one JSON line per case; --out FILE appends them there; --load S (default 1.0 for case118, 0.5 otherwise); --max-iter K (default
200); --tr-size D (default 0.4)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import acopf  # noqa: E402


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
    info = opt.lm_info()
    opt.close()
    return ms, run, info


def emit(out):
    line = json.dumps(out)
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write(line + "\n")


def runs(case):
    reps, max_iter, tr_size, memory = arg("--reps", 5), arg("--max-iter", 200), arg("--tr-size", 0.4), arg("--memory", 10)
    load = arg("--load", 1.0 if case == "case118" else 0.5)
    grid = acopf.synthetic_case(case, 1, load)
    ohm, expr = acopf.function_model(grid), acopf.function_model(grid, nlp="expr")
    kw = dict(max_iter=max_iter, tr_size=tr_size, device_eval=True)
    setups = {"tr": (ohm, A.Parameters(algorithm="Trust Region", **kw)),
              "eqp_lm": (ohm, A.Parameters(algorithm="SLP-EQP", hessian_type="limited-memory", lm_memory=memory, **kw)),
              "eqp_exact": (expr, A.Parameters(algorithm="SLP-EQP", **kw))}
    prs = {k: fm.to_problem("%s-sized" % case) for k, (fm, _) in setups.items()}
    ms, last = {k: [] for k in setups}, {}
    for k, (fm, par) in setups.items():              # code objects, pinned staging: not part of any timing
        one_run(fm, prs[k], par)
    order = list(setups) + list(setups)[::-1]
    for _ in range(reps):
        for k in order:
            t, run, info = one_run(setups[k][0], prs[k], setups[k][1])
            ms[k].append(t)
            last[k] = (run, info)
    out = dict(mode="runs", case=case, load=load, n=int(prs["tr"].n), m=int(prs["tr"].m), max_iter=max_iter, tr_size=tr_size, memory=memory, reps=2 * reps)
    for k, (r, info) in last.items():
        out[k] = dict(status=r.ret, iter=r.iter, lp_solves=r.lp_solves, restoration_solves=r.restoration_solves, obj_val=r.obj_val, prim_infeas=r.prim_infeas,
                      dual_infeas=r.dual_infeas, compl=r.compl, ms_median=float(np.median(ms[k])), ms_min=float(min(ms[k])), ms_max=float(max(ms[k])))
        if r.eqp_counts is not None:
            out[k].update(counts=r.eqp_counts, radius=r.Delta_E)
    info = last["eqp_lm"][1]
    out["eqp_lm"]["lm_info"] = dict(memory=info.memory, pairs=info.pairs, pushed=info.pushed, skipped_zero=info.skipped_zero,
                                    skipped_curvature=info.skipped_curvature, sigma=info.sigma, bytes=info.bytes)
    emit(out)


def products(case):
    reps, memory = arg("--reps", 5), arg("--memory", 10)
    grid = acopf.synthetic_case(case, 1, arg("--load", 1.0 if case == "case118" else 0.5))
    out = dict(mode="products", case=case, memory=memory, reps=reps)
    rng = np.random.default_rng(1)
    for key, fm in (("lm", acopf.function_model(grid)), ("exact", acopf.function_model(grid, nlp="expr"))):
        pr = fm.to_problem(case)
        n, m = int(pr.n), int(pr.m)
        opt = handle(fm, pr)
        opt.set_kkt_form("sparse")                   # (no dense Jacobian of the solve's own: nothing here reads one)
        x = np.clip(pr.x0, pr.x_L, pr.x_U)
        _, df, _ = opt.eval_functions(x)
        if key == "lm":
            opt.set_hessian_type("limited-memory", memory)
            for _ in range(memory):                  # pairs of a diagonal positive definite matrix
                s = rng.standard_normal(n)
                opt.lm_push_pair(s, s * np.linspace(1.0, 10.0, n))
        lam, rs, bs = np.zeros(m), np.zeros(m, np.int32), np.zeros(n, np.int32)
        RU, RW, radii = np.tile(df, (64, 1)), np.zeros((64, m)), 0.4 * np.linspace(0.05, 1.5, 64)
        calls = dict(one=lambda: opt.kkt_step(x, lam, rs, bs, df, np.zeros(m), 0.4, max_iter=20, rtol=1e-12, normal_share=0.8),
                     multi64=lambda: opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii, max_iter=20, rtol=1e-12, normal_share=0.8))
        res = {}
        for name, fn in calls.items():
            got = fn()
            infos = got[3] if isinstance(got[3], list) else [got[3]]
            t = []
            for _ in range(reps):
                t0 = time.perf_counter()
                fn()
                t.append(1e3 * (time.perf_counter() - t0))
            res[name] = dict(call_ms_median=float(np.median(t)), call_ms_min=float(min(t)), call_ms_max=float(max(t)), cg_iters_max=int(max(i.cg_iters for i in infos)))
        if key == "lm":
            V = rng.standard_normal((64, n))
            for name, W in (("lm_product_1", V[:1]), ("lm_product_64", V)):
                opt.lm_product(W)
                t = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    opt.lm_product(W)
                    t.append(1e3 * (time.perf_counter() - t0))
                res[name] = dict(call_ms_median=float(np.median(t)), call_ms_min=float(min(t)), call_ms_max=float(max(t)))
            res["bytes"] = int(opt.lm_info().bytes)
        out[key] = dict(res, n=n, m=m)
        opt.close()
    emit(out)


def main():
    if "--products" in sys.argv:
        for case in arg("--products", "").split(","):
            products(case)
    else:
        for case in arg("--cases", "case118").split(","):
            runs(case)


if __name__ == "__main__":
    main()
