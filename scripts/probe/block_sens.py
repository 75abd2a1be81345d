"""The data derivatives of the Ohm's-law kernel (nlp_kind 4, acopf.function_model(case, hessian=True)) beside those of the expression form
with the branch coefficients as parameters (nlp="expr", branch_params=True) on the same build: case118- and case1354pegase-sized grids
(load scale 0.5), each at the point a short Line Search asm_slp_run of the kernel form reaches, on the working set of its multipliers.
Two handles per case in one process; the forms alternate call by call (block, expr, block, ...), so that both see the same clocks.
The expression form is the comparator: it is what the entries ran on before the block kernels had them.  Timed, after a warm-up call,
--reps (5) repeats on the host clock, every call ending with its results on the host; all repeats are printed, with median and spread
(max - min):
    data_gradient       asm_eval_data_gradient
    data_cross          asm_eval_data_cross
    sens_multi_64       asm_solution_sensitivity_multi with 64 random directions (sparse KKT form)
    sens_multi_64_zero  the same call on 64 zero directions: the same launches for the right-hand sides, no conjugate-gradient round
    kkt_multi_64        asm_kkt_solve_multi fed with the 64 pairs (u, w) of those directions: the same solve without making them
rhs_ms = median(sens_multi_64) - median(kkt_multi_64) is the right-hand-side part of the call (the directions' upload and the
cross-derivative launches against the upload of finished right-hand sides); cg_ms = median(sens_multi_64) - median(sens_multi_64_zero) is
what the call spends in the iteration.

This file is the parent; every case runs in a child process of its own under `timeout` (--case NAME runs one case in this process), so
that a case that takes too long ends alone.  Prints one JSON line per case; --out FILE appends them there."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = ("case118", "case1354pegase")
LIMIT_S = {"case118": 150, "case1354pegase": 420}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def run_case(name, reps):
    import activesetmethods_amd as A
    from activesetmethods_amd import acopf, sensitivity
    case = acopf.synthetic_case(name, 1, 0.5)
    fms = dict(block=acopf.function_model(case, hessian=True), expr=acopf.function_model(case, nlp="expr", branch_params=True))
    pr = fms["block"].to_problem(name)
    opts = {}
    for form, fm in fms.items():
        p = fm.to_problem(name)
        opts[form] = A.HipSubOptimizer(A.QpData(np.zeros(p.n), 0.0, np.zeros(p.nnz), np.zeros(p.m), p.g_L, p.g_U, p.x_L, p.x_U), p.j_row, p.j_col)
        opts[form].eval_setup(fm)
        opts[form].set_kkt_form("sparse")
    run = opts["block"].slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    if rs.sum() > (bs == 0).sum():
        rs[np.nonzero(rs)[0][int((bs == 0).sum()):]] = 0
    nd = len(fms["block"].nlp.device[2])
    assert len(fms["expr"].nlp.device[2]) == nd
    rng = np.random.default_rng(9)
    DC, Z = rng.standard_normal((64, nd)), np.zeros((64, nd))
    out = dict(case=name, n=int(pr.n), m=int(pr.m), n_dpar=nd, n_rows=int(rs.sum()), n_free=int((bs == 0).sum()), reps=reps)
    calls, res = {}, {}
    for form, opt in opts.items():
        UW = [opt.data_cross(x, lam, dc) for dc in DC]
        RU, RW = np.stack([u for u, _ in UW]), np.stack([w for _, w in UW])
        calls[form] = dict(data_gradient=lambda o=opt: o.eval_data_gradient(x, lam), data_cross=lambda o=opt: o.data_cross(x, lam, DC[0]),
                           sens_multi_64=lambda o=opt: o.solution_sensitivity_multi(x, lam, rs, bs, DC),
                           sens_multi_64_zero=lambda o=opt: o.solution_sensitivity_multi(x, lam, rs, bs, Z),
                           kkt_multi_64=lambda o=opt, a=RU, b=RW: o.kkt_solve_multi(x, lam, rs, bs, a, b))
        res[form] = {k: dict(ms=[]) for k in calls[form]}
    for key in calls["block"]:
        for form in calls:                     # warm-up
            got = calls[form][key]()
            if key.endswith("_64"):
                res[form][key]["rounds"] = int(max(i.cg_iters for i in got[3]))
                res[form][key]["statuses"] = sorted({int(i.status) for i in got[3]})
        for _ in range(reps):                  # the forms alternate
            for form in calls:
                ms, _ = timed(calls[form][key])
                res[form][key]["ms"].append(ms)
    for form in calls:
        for key, r in res[form].items():
            r["median"] = float(np.median(r["ms"]))
            r["spread"] = float(max(r["ms"]) - min(r["ms"]))
        res[form]["rhs_ms"] = res[form]["sens_multi_64"]["median"] - res[form]["kkt_multi_64"]["median"]
        res[form]["cg_ms"] = res[form]["sens_multi_64"]["median"] - res[form]["sens_multi_64_zero"]["median"]
    # the two forms' answers, for the record
    gb, ge = calls["block"]["data_gradient"](), calls["expr"]["data_gradient"]()
    sb, se = calls["block"]["sens_multi_64"](), calls["expr"]["sens_multi_64"]()
    out["max_rel_diff_gradient"] = float(np.abs(gb - ge).max() / max(1.0, np.abs(ge).max()))
    out["max_rel_diff_DX"] = float(np.abs(sb[0] - se[0]).max() / max(1.0, np.abs(se[0]).max()))
    out.update(res)
    for opt in opts.values():
        opt.close()
    return out


def main():
    reps = arg("--reps", 5)
    if "--case" in sys.argv:
        line = json.dumps(run_case(arg("--case", ""), reps))
        print(line)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(line + "\n")
        return 0
    names = [c for c in CASES if c in sys.argv] or list(CASES)
    for name in names:
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(reps)]
        if "--out" in sys.argv:
            cmd += ["--out", arg("--out", "")]
        rc = subprocess.run(cmd).returncode
        if rc != 0:                            # a fault, an abort or a time limit: nothing more is started on the device
            print("%s ended with status %d: stopping" % (name, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
