"""Times of the KKT entries on the case300-sized expression ACOPF with branch parameters (load scale 0.5) at its SLP solution, the instance
of sens_multi.py: asm_solution_sensitivity_multi at 64 columns and one asm_solution_sensitivity call, and - where the build has them -
asm_kkt_step_multi on a 64-rung radius ladder of one right-hand side beside 64 asm_kkt_step calls on the same rungs.  Runs on a build
without the step entries too, so that the same probe times the entries both builds share.  Per figure: warm-up, then --reps (5) repeats
on the host clock, every call ending with its results on the host; all repeats are printed, with median and spread (max - min).
Prints one JSON line; --out FILE also writes it there."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import acopf, sensitivity  # noqa: E402


def repeats(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return dict(ms=ts, median=float(np.median(ts)), spread=max(ts) - min(ts))


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 5
    fm = acopf.function_model(acopf.synthetic_case("case300", 1, 0.5), nlp="expr", branch_params=True)
    pr = fm.to_problem("case300 branch parameters")
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=200, device_eval=True), 0)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    DC = np.random.default_rng(1).standard_normal((64, len(fm.nlp.device[2])))
    out = dict(case="case300", load_scale=0.5, n=pr.n, m=pr.m, slp_ret=int(run.ret), reps=reps, has_step=hasattr(opt, "kkt_step_multi"))
    out["sensitivity_multi_64"] = repeats(lambda: opt.solution_sensitivity_multi(x, lam, rs, bs, DC), reps)
    out["sensitivity_single"] = repeats(lambda: opt.solution_sensitivity(x, lam, rs, bs, DC[0]), reps)
    if out["has_step"]:
        ru, rw = opt.data_cross(x, lam, DC[0])
        full = opt.kkt_solve(x, lam, rs, bs, ru, rw)
        radii = float(np.linalg.norm(full[0])) * np.linspace(0.05, 1.5, 64)
        RU, RW = np.tile(ru, (64, 1)), np.tile(rw, (64, 1))
        multi = opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii)
        single = [opt.kkt_step(x, lam, rs, bs, ru, rw, r) for r in radii]
        out["ladder"] = dict(full_cg_iters=int(full[3].cg_iters), boundary=[int(i.boundary) for i in multi[3]], cg_iters=[int(i.cg_iters) for i in multi[3]],
                             same_decisions=all(m.boundary == s[3].boundary and m.cg_iters == s[3].cg_iters for m, s in zip(multi[3], single)),
                             max_rel_diff_to_single=max(float(np.abs(multi[0][c] - single[c][0]).max() / max(1.0, np.abs(single[c][0]).max())) for c in range(64)))
        out["step_multi_ladder_64"] = repeats(lambda: opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii), reps)
        out["step_single_x64"] = repeats(lambda: [opt.kkt_step(x, lam, rs, bs, ru, rw, r) for r in radii], reps)
        out["solve_multi_64_same_rhs"] = repeats(lambda: opt.kkt_solve_multi(x, lam, rs, bs, RU, RW), reps)
    opt.close()
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
