"""64 variable-bound columns through asm_var_bound_sensitivity_multi (right-hand sides made on the device from 12 bytes per column) beside
the same columns through asm_kkt_solve_multi with right-hand sides made on the host (RU[c] = delta[c] H[:, j], RW[c] = delta[c] J[:, j],
staged as n- and m-long rows), on the case300-sized ACOPF (load scale 0.5) on the Ohm's-law kernel with derivatives, at the point a short
Line Search asm_slp_run reaches, on the working set of its multipliers.  The variables are those the point leaves at a bound - where it
leaves fewer than eight, the first free voltage magnitudes join B (a working set is a statement about the linear algebra) - repeated
with seeded moves up to 64 columns; --kkt-form (dense) is the form of every solve.
One handle; the routes alternate call by call, so that both see the same clocks.  Timed after a warm-up call of each, on the host clock,
every call ending with its results on the host; all repeats are printed, with median and spread (max - min):
    device       asm_var_bound_sensitivity_multi(vars, delta)                         --reps (9) repeats
    given        asm_kkt_solve_multi on RU, RW that are already in host memory        --reps repeats
    host_rhs     making RU, RW on the host: one asm_eval_hessian_product per distinct variable and the Jacobian values, once per repeat
Cross-check: DLAM, DZ and DX (but DX[c, j] = delta[c]) of the two routes, largest absolute difference (0.0: the same bits).

This file is the parent; the case runs in a child process under `timeout` (--child runs it in this process), so that a run that takes
too long ends alone.  Prints one JSON line; --out FILE appends it there."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
LIMIT_S = 300
NCOL = 64


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def host_rhs(opt, pr, x, lam, vars, delta):
    opt.eval_functions(x)
    J = np.zeros((pr.m, pr.n))
    np.add.at(J, (np.asarray(opt.j_row) - 1, np.asarray(opt.j_col) - 1), opt.jacobian_values())
    cols = {}
    for j in sorted(set(vars.tolist())):
        e = np.zeros(pr.n)
        e[j] = 1.0
        cols[j] = opt.hessian_product(x, 1.0, -lam, e)
    RU = np.stack([delta[c] * cols[int(j)] for c, j in enumerate(vars)])
    RW = np.stack([delta[c] * J[:, j] for c, j in enumerate(vars)])
    return RU, RW


def run_case(name, reps, kkt_form):
    import activesetmethods_amd as A
    from activesetmethods_amd import acopf, sensitivity
    fm = acopf.function_model(acopf.synthetic_case(name, 1, 0.5), hessian=True)
    pr = fm.to_problem(name)
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    opt.set_kkt_form(kkt_form)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    if rs.sum() > (bs == 0).sum():
        rs[np.nonzero(rs)[0][int((bs == 0).sum()):]] = 0
    own = int((bs != 0).sum())
    for j in fm.acopf_model.vm:
        if (bs != 0).sum() >= 8 or (bs == 0).sum() - 1 < rs.sum():
            break
        if bs[j] == 0:
            bs[j] = -1
    B = np.nonzero(bs != 0)[0]
    vars = np.array([int(B[c % len(B)]) for c in range(NCOL)], np.int32)
    delta = 0.25 + np.random.default_rng(9).uniform(-2.0, 2.0, NCOL)
    out = dict(case=name, kkt_form=kkt_form, n=int(pr.n), m=int(pr.m), n_rows=int(rs.sum()), n_free=int((bs == 0).sum()), n_bound=int(len(B)), n_bound_of_the_point=own,
               columns=NCOL, reps=reps, form_used=None)
    RU, RW = host_rhs(opt, pr, x, lam, vars, delta)
    calls = dict(device=lambda: opt.var_bound_sensitivity_multi(x, lam, rs, bs, vars, delta), given=lambda: opt.kkt_solve_multi(x, lam, rs, bs, RU, RW),
                 host_rhs=lambda: host_rhs(opt, pr, x, lam, vars, delta))
    res = {k: dict(ms=[]) for k in calls}
    got = {k: calls[k]() for k in calls}                       # warm-up
    out["form_used"] = int(opt.kkt_form_info().form_used)
    for k in ("device", "given"):
        res[k].update(statuses=sorted({int(i.status) for i in got[k][3]}), cg_iters=sorted({int(i.cg_iters) for i in got[k][3]}))
    for _ in range(reps):                                      # the routes alternate
        for k in calls:
            ms, _ = timed(calls[k])
            res[k]["ms"].append(ms)
    for k in calls:
        res[k]["median"] = float(np.median(res[k]["ms"]))
        res[k]["spread"] = float(max(res[k]["ms"]) - min(res[k]["ms"]))
    dev, giv = got["device"], got["given"]
    dx = dev[0].copy()
    dx[np.arange(NCOL), vars] = giv[0][np.arange(NCOL), vars]
    out["moved_entries_are_delta"] = bool(np.array_equal(dev[0][np.arange(NCOL), vars], delta))
    out["max_abs_diff"] = dict(dx=float(np.abs(dx - giv[0]).max()), dlam=float(np.abs(dev[1] - giv[1]).max()), dz=float(np.abs(dev[2] - giv[2]).max()))
    out["given_over_device"] = res["given"]["median"] / res["device"]["median"]
    out.update(res)
    opt.close()
    return out


def main():
    reps, form, name = arg("--reps", 9), arg("--kkt-form", "dense"), arg("--case", "case300")
    if "--child" in sys.argv:
        line = json.dumps(run_case(name, reps, form))
        print(line)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(line + "\n")
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", "--case", name, "--reps", str(reps), "--kkt-form", form]
    if "--out" in sys.argv:
        cmd += ["--out", arg("--out", "")]
    rc = subprocess.run(cmd).returncode
    if rc != 0:                                # a fault, an abort or a time limit: nothing more is started on the device
        print("%s ended with status %d" % (name, rc))
    return rc


if __name__ == "__main__":
    sys.exit(main())
