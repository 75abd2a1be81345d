"""Expression block (nlp_kind 3) against the hand-written Ohm's-law kernel (nlp_kind 1) at C4 size (case1354pegase-sized, load scale 0.5)
(GPU): a full asm_eval_functions of each, alternating, on synchronised host clocks (the call ends with a stream synchronise); then a
20-LP native Line Search run (asm_slp_run on a handle set up beforehand, warm state reset) of each, alternating.  Prints one JSON line; --out FILE also writes it there."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import acopf  # noqa: E402


def handle(pr):
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(pr.function_model)
    return opt


def main():
    reps, lps, rounds = 200, 20, 6
    case = acopf.synthetic_case("case1354pegase", 1, 0.5)
    prs = {k: acopf.function_model(case, nlp=k).to_problem("c4 " + k) for k in ("expr", "acopf_ohm")}
    out = dict(case="case1354pegase", load_scale=0.5, n=prs["expr"].n, m=prs["expr"].m, nodes=int(prs["expr"].function_model.nlp.tape.L))
    # ---- full evaluation
    opts = {k: handle(pr) for k, pr in prs.items()}
    x = prs["expr"].x0 + 0.01 * np.random.default_rng(1).standard_normal(prs["expr"].n)
    for o in opts.values():
        for _ in range(10):
            o.eval_functions(x)
    ev = {k: [] for k in opts}
    for _ in range(reps):
        for k, o in opts.items():
            t0 = time.perf_counter()
            o.eval_functions(x)
            ev[k].append(time.perf_counter() - t0)
    for k, o in opts.items():
        o.close()
        out["eval_ms_median_" + k] = 1e3 * float(np.median(ev[k]))
        out["eval_ms_p10_" + k] = 1e3 * float(np.percentile(ev[k], 10))
    # ---- native C4 run, 20 LPs: asm_slp_run on a handle made beforehand (setup not timed), the kinds alternating
    import ctypes as C
    from activesetmethods_amd import _lib, batch
    lib = _lib.load()
    par = batch.slp_params(A.Parameters(algorithm="Line Search", max_iter=10 ** 6, device_eval=True), lps)
    step, xs = {k: [] for k in prs}, {}
    opts = {k: handle(pr) for k, pr in prs.items()}
    for _ in range(rounds):
        for k, pr in prs.items():
            o = opts[k]
            x0 = np.ascontiguousarray(pr.x0, np.float64)
            xo = np.empty(pr.n)
            res = _lib.SlpResult()
            assert lib.asm_sublp_reset_warm(o._h) == 0
            t0 = time.perf_counter()
            rc = lib.asm_slp_run(o._h, C.byref(par), _lib.dptr(x0), _lib.dptr(xo), None, None, None, None, C.byref(res))
            dt = time.perf_counter() - t0
            assert rc == 0, lib.asm_last_error(o._h)
            step[k].append(1e3 * dt / max(res.lp_solves, 1))
            out["lp_solves_" + k] = int(res.lp_solves)
            xs[k] = xo
    for o in opts.values():
        o.close()
    out["run_max_abs_x_diff"] = float(np.abs(xs["expr"] - xs["acopf_ohm"]).max())
    for k in prs:
        out["native_ms_per_lp_" + k] = step[k]
        out["native_ms_per_lp_median_" + k] = float(np.median(step[k]))
    out["native_ratio_expr_over_ohm"] = out["native_ms_per_lp_median_expr"] / out["native_ms_per_lp_median_acopf_ohm"]
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
