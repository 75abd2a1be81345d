"""Solution sensitivity of the case300-sized expression ACOPF with branch parameters (load scale 0.5) at its SLP solution on the GPU:
one asm_solution_sensitivity beside asm_eval_data_cross alone and asm_kkt_solve stopped before its first CG iteration (max_iter 0:
evaluation, gather, rank-K build, factorisation, particular solution, multipliers and residuals - everything but the iterations),
alternating, on synchronised host clocks (each call ends with a stream synchronise and its copies back to the host).
Prints one JSON line; --out FILE also writes it there."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import acopf, sensitivity  # noqa: E402


def main():
    reps = 30
    fm = acopf.function_model(acopf.synthetic_case("case300", 1, 0.5), nlp="expr", branch_params=True)
    pr = fm.to_problem("case300 branch parameters")
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=200, device_eval=True), 0)
    rs, bs = sensitivity.working_set(pr, run.x, run.lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    dc = np.random.default_rng(1).standard_normal(len(fm.nlp.device[2]))
    t0 = time.perf_counter()
    dx, dlam, dz, info = opt.solution_sensitivity(run.x, run.lam, rs, bs, dc)          # the first call builds lists and buffers
    first_ms = 1e3 * (time.perf_counter() - t0)
    u, w = opt.data_cross(run.x, run.lam, dc)
    out = dict(case="case300", load_scale=0.5, n=pr.n, m=pr.m, n_dpar=len(dc), slp_ret=int(run.ret), slp_lp_solves=int(run.lp_solves), n_free=int(info.n_free),
               n_rows=int(info.n_rows), status=int(info.status), cg_iters=int(info.cg_iters), dropped_pivots=int(info.dropped_pivots),
               res_stat=float(info.res_stat), res_feas=float(info.res_feas), max_dx=float(np.abs(dx).max()), max_dlam=float(np.abs(dlam).max()), first_call_ms=first_ms)
    calls = {"solution_sensitivity": lambda: opt.solution_sensitivity(run.x, run.lam, rs, bs, dc),
             "kkt_without_iterations": lambda: opt.kkt_solve(run.x, run.lam, rs, bs, u, w, max_iter=0, rtol=1e-12),
             "data_cross": lambda: opt.data_cross(run.x, run.lam, dc)}
    for fn in calls.values():
        for _ in range(3):
            fn()
    ts = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append(time.perf_counter() - t0)
    opt.close()
    for k in calls:
        out[k + "_ms_median"] = 1e3 * float(np.median(ts[k]))
        out[k + "_ms_p10"] = 1e3 * float(np.percentile(ts[k], 10))
    it = out["solution_sensitivity_ms_median"] - out["kkt_without_iterations_ms_median"] - out["data_cross_ms_median"]
    out["cg_iterations_ms"] = it
    out["cg_share"] = it / out["solution_sensitivity_ms_median"]
    out["ms_per_cg_iteration"] = it / max(out["cg_iters"], 1)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
