"""Hessian of the Lagrangian of the C4-sized expression model (case1354pegase-sized, load scale 0.5) on the GPU: one
asm_eval_hessian_lagrangian and one asm_eval_hessian_product beside the first-order full evaluation (asm_eval_functions) of the same
handle, alternating, on synchronised host clocks (each call ends with a stream synchronise and its copy back to the host).
Prints one JSON line; --out FILE also writes it there."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import acopf  # noqa: E402


def main():
    reps = 200
    fm = acopf.function_model(acopf.synthetic_case("case1354pegase", 1, 0.5), nlp="expr")
    pr = fm.to_problem("c4 expr")
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    rng = np.random.default_rng(1)
    x = pr.x0 + 0.01 * rng.standard_normal(pr.n)
    lam, v = rng.standard_normal(pr.m), rng.standard_normal(pr.n)
    t0 = time.perf_counter()
    rows, _ = opt.hessian_structure()                       # the first call builds pattern, lists and workspace
    first_ms = 1e3 * (time.perf_counter() - t0)
    sweep = fm.nlp._hess_prepare()["sweep"]
    out = dict(case="case1354pegase", load_scale=0.5, n=pr.n, m=pr.m, nodes=int(fm.nlp.tape.L), rows_and_terms=int(fm.nlp.tape.R + fm.nlp.tape.T),
               hess_nnz=int(len(rows)), seed_threads=int(sweep.nr), workspace_nodes=int(sweep.lens.sum()),
               workspace_mb=4 * 8 * float(sweep.lens.sum()) / 2 ** 20, first_call_ms=first_ms)
    calls = {"eval_functions": lambda: opt.eval_functions(x), "hessian_lagrangian": lambda: opt.eval_hessian_lagrangian(x, 1.0, lam),
             "hessian_product": lambda: opt.hessian_product(x, 1.0, lam, v)}
    for fn in calls.values():
        for _ in range(10):
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
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
