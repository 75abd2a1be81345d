"""SLP-EQP against the Trust-Region SLP, both whole inside the library (asm_slp_run_eqp, asm_slp_run_tr) on the same build: iterations,
LP solves, the EQP counters and the wall time of a run on the case118-sized and case300-sized ACOPF with the Ohm's-law rows as
expressions (nlp="expr": the model has second derivatives).  Every run starts on a fresh handle (set-up outside the clock); the clock
is the host's around one C call, which ends with its results on the host.  One warm-up run of each driver, then --reps (default 5)
rounds in ABBA order.  Prints one JSON line per case; --out FILE appends them there; --cases a,b (default case118,case300);
--load S (default: 1.0 for case118, 0.5 for case300); --max-iter K (default 200); --tr-size D (default 0.4, the LP's initial radius and
the step's)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import acopf  # noqa: E402

LOADS = {"case118": 1.0, "case300": 0.5}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def one_run(fm, pr, par):
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    t0 = time.perf_counter()
    run = opt.slp_run(pr.x0, par)
    ms = 1e3 * (time.perf_counter() - t0)
    opt.close()
    return ms, run


def main():
    reps, max_iter, tr_size = arg("--reps", 5), arg("--max-iter", 200), arg("--tr-size", 0.4)
    for case in arg("--cases", "case118,case300").split(","):
        load = arg("--load", LOADS.get(case, 1.0))
        fm = acopf.function_model(acopf.synthetic_case(case, 1, load), nlp="expr")
        pr = fm.to_problem("%s-sized" % case)
        pars = {"eqp": A.Parameters(algorithm="SLP-EQP", max_iter=max_iter, tr_size=tr_size, device_eval=True),
                "tr": A.Parameters(algorithm="Trust Region", max_iter=max_iter, tr_size=tr_size, device_eval=True)}
        ms, last = {k: [] for k in pars}, {}
        for k in pars:                                  # code objects, pinned staging: not part of either timing
            one_run(fm, pr, pars[k])
        for _ in range(reps):
            for k in ("eqp", "tr", "tr", "eqp"):
                t, last[k] = one_run(fm, pr, pars[k])
                ms[k].append(t)
        out = dict(case=case, load=load, n=pr.n, m=pr.m, max_iter=max_iter, tr_size=tr_size, reps=2 * reps)
        for k, r in last.items():
            out[k] = dict(status=r.ret, iter=r.iter, lp_solves=r.lp_solves, restoration_solves=r.restoration_solves, obj_val=r.obj_val,
                          prim_infeas=r.prim_infeas, dual_infeas=r.dual_infeas, compl=r.compl, delta=r.delta, accepted=r.accepted, rejected=r.rejected,
                          ms_median=float(np.median(ms[k])), ms_p10=float(np.percentile(ms[k], 10)), ms_p90=float(np.percentile(ms[k], 90)),
                          ms_per_iter=float(np.median(ms[k])) / max(r.iter, 1))
        out["eqp"].update(counts=last["eqp"].eqp_counts, radius=last["eqp"].Delta_E)
        line = json.dumps(out)
        print(line, flush=True)
        if "--out" in sys.argv:
            with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
