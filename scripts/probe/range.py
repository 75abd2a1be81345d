"""The validity ranges of 64 bound-sensitivity columns through asm_sensitivity_range_multi beside the host route a caller had before it
(sensitivity.validity_range_host: the dense m x n Jacobian from the model's callbacks, V = J dx per column and the ratio tests in NumPy),
on the case118- and case300-sized ACOPF (load scale 0.5) on the Ohm's-law kernel with derivatives, at the point a short Line Search
asm_slp_run reaches, on the working set of its multipliers.  The columns are asm_bound_sensitivity_multi's for the first working rows
(sparse KKT form), repeated with seeded moves up to 64.
One handle per case; the two routes alternate call by call, so that both see the same clocks.  Timed after a warm-up call of each, on the
host clock, every call ending with its results on the host; all repeats are printed, with median and spread (max - min):
    device   asm_sensitivity_range_multi on the 64 columns: the evaluation at x, the assembly, one upload, two launches, one read-back
    host     dense_jacobian plus the NumPy twin
    host_j   dense_jacobian alone (the part of `host` that builds the m x n matrix)
Cross-check: the largest relative difference of a finite t, the (position, kind) pairs that differ, the kinds that block.

This file is the parent; each case runs in a child process under `timeout` (--child runs it in this process), so that a run that takes
too long ends alone and nothing is started after it.  Prints one JSON line per case; --out FILE appends them there."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
LIMIT_S = 420
NCOL = 64


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def run_case(name, reps):
    import activesetmethods_amd as A
    from activesetmethods_amd import acopf, sensitivity
    fm = acopf.function_model(acopf.synthetic_case(name, 1, 0.5), hessian=True)
    pr = fm.to_problem(name)
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    opt.set_kkt_form("sparse")
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    if rs.sum() > (bs == 0).sum():
        rs[np.nonzero(rs)[0][int((bs == 0).sum()):]] = 0
    W = np.nonzero(rs)[0]
    rows = np.array([int(W[c % len(W)]) for c in range(NCOL)], np.int32)
    delta = 0.25 + np.random.default_rng(9).uniform(-2.0, 2.0, NCOL)
    DX, DLAM, DZ, infos = opt.bound_sensitivity_multi(x, lam, rs, bs, rows, delta)
    point = (x, lam, run.mult_x_U, run.mult_x_L, rs, bs)
    out = dict(case=name, n=int(pr.n), m=int(pr.m), nnz=int(pr.nnz), n_rows=int(rs.sum()), n_bound=int((bs != 0).sum()), columns=NCOL, reps=reps,
               column_statuses=sorted({int(i.status) for i in infos}), dense_jacobian_mb=8e-6 * pr.m * pr.n)
    calls = dict(device=lambda: opt.sensitivity_range(*point, DX, DLAM, DZ), host=lambda: sensitivity.validity_range_host(pr, *point, DX, DLAM, DZ),
                 host_j=lambda: sensitivity.dense_jacobian(fm, x))
    res = {k: dict(ms=[]) for k in calls}
    got = {k: calls[k]() for k in calls}                       # warm-up
    for _ in range(reps):                                      # the routes alternate
        for k in calls:
            ms, _ = timed(calls[k])
            res[k]["ms"].append(ms)
    for k in calls:
        res[k]["median"] = float(np.median(res[k]["ms"]))
        res[k]["spread"] = float(max(res[k]["ms"]) - min(res[k]["ms"]))
    dev, host = got["device"], got["host"]
    worst, differ = 0.0, 0
    for side in ("lo", "hi"):
        td, th = dev["t_" + side], host["t_" + side]
        fin = np.isfinite(th)
        assert np.array_equal(fin, np.isfinite(td))
        nz = fin & (th != 0.0)
        if nz.any():
            worst = max(worst, float(np.max(np.abs(td[nz] - th[nz]) / np.abs(th[nz]))))
        differ += int(np.sum((dev["pos_" + side] != host["pos_" + side]) | (dev["kind_" + side] != host["kind_" + side])))
    out["max_rel_diff_t"], out["blockers_that_differ"] = worst, differ
    out["kinds"] = sorted(set(dev["kind_lo"].tolist()) | set(dev["kind_hi"].tolist()))
    out["finite_sides"] = int(np.isfinite(dev["t_lo"]).sum() + np.isfinite(dev["t_hi"]).sum())
    out["host_over_device"] = res["host"]["median"] / res["device"]["median"]
    out.update(res)
    opt.close()
    return out


def main():
    reps = arg("--reps", 9)
    if "--child" in sys.argv:
        line = json.dumps(run_case(arg("--case", "case118"), reps))
        print(line)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(line + "\n")
        return 0
    for name in ((arg("--case", ""),) if "--case" in sys.argv else ("case118", "case300")):
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", "--case", name, "--reps", str(reps)]
        if "--out" in sys.argv:
            cmd += ["--out", arg("--out", "")]
        rc = subprocess.run(cmd).returncode
        if rc != 0:                                # a fault, an abort or a time limit: nothing more is started on the device
            print("%s ended with status %d" % (name, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
