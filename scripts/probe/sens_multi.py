"""Sensitivity matrices of the case300-sized expression ACOPF with branch parameters (load scale 0.5) at its SLP solution on the GPU:
asm_solution_sensitivity_multi at nrhs = 1, 8, 32, 64 beside a loop of nrhs asm_solution_sensitivity calls on the same directions, in the
same process.  The comparator is the single-column entry, whose code the multi entry does not touch.  Per nrhs: warm-up, then the two in
alternating (ABBA) order on host clocks - every call ends with a stream synchronise and its copies back to the host - median and 10th
percentile; the multi call stopped before its first iteration (max_iter 0) gives the time outside the iterations, and the rest over the
largest cg_iters of the call the time of one lockstep round.  The two answers are compared in the same run.
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
    reps = 8
    fm = acopf.function_model(acopf.synthetic_case("case300", 1, 0.5), nlp="expr", branch_params=True)
    pr = fm.to_problem("case300 branch parameters")
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=200, device_eval=True), 0)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    nd = len(fm.nlp.device[2])
    DC = np.random.default_rng(1).standard_normal((64, nd))
    out = dict(case="case300", load_scale=0.5, n=pr.n, m=pr.m, n_dpar=nd, slp_ret=int(run.ret), slp_lp_solves=int(run.lp_solves), reps=reps, rows=[])
    for nrhs in (1, 8, 32, 64):
        D = np.ascontiguousarray(DC[:nrhs])
        multi = lambda: opt.solution_sensitivity_multi(x, lam, rs, bs, D)
        loop = lambda: [opt.solution_sensitivity(x, lam, rs, bs, D[c]) for c in range(nrhs)]
        noiter = lambda: opt.solution_sensitivity_multi(x, lam, rs, bs, D, max_iter=0, rtol=1e-12)
        got, ref = multi(), loop()                               # (the first calls build lists and buffers)
        multi(), noiter()
        diff = max(float(np.abs(got[k][c] - ref[c][k]).max() / max(1.0, np.abs(ref[c][k]).max())) for c in range(nrhs) for k in range(3))
        ts = {"multi": [], "loop": [], "noiter": []}

        def timed(name, fn):
            t0 = time.perf_counter()
            fn()
            ts[name].append(time.perf_counter() - t0)
        for r in range(reps):
            order = (("multi", multi), ("loop", loop)) if r % 2 == 0 else (("loop", loop), ("multi", multi))
            for name, fn in order + order[::-1]:
                timed(name, fn)
            timed("noiter", noiter)
        iters = [int(i.cg_iters) for i in got[3]]
        row = dict(nrhs=nrhs, status=sorted({int(i.status) for i in got[3]}), cg_iters_max=max(iters), cg_iters_min=min(iters),
                   single_cg_iters_max=max(int(r_[3].cg_iters) for r_ in ref), n_free=int(got[3][0].n_free), n_rows=int(got[3][0].n_rows),
                   max_rel_diff_to_single=diff, res_stat_max=max(float(i.res_stat) for i in got[3]), res_feas_max=max(float(i.res_feas) for i in got[3]))
        for k in ts:
            row[k + "_ms_median"] = 1e3 * float(np.median(ts[k]))
            row[k + "_ms_p10"] = 1e3 * float(np.percentile(ts[k], 10))
        row["speedup_median"] = row["loop_ms_median"] / row["multi_ms_median"]
        row["ms_per_round"] = (row["multi_ms_median"] - row["noiter_ms_median"]) / max(row["cg_iters_max"], 1)
        out["rows"].append(row)
    opt.close()
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
