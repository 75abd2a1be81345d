"""The adjoint route to the gradient of one function of the solution with respect to ALL constants of the model (asm_solution_adjoint: one
KKT solve and one transposed cross-derivative sweep) beside the forward route on the same build (ceil(n_dpar / 64)
asm_solution_sensitivity_multi calls on unit directions, each contracted with the function's gradients gx, gl), on the case300-sized
ACOPF (load scale 0.5) in both its forms: the expression form with the branch coefficients as parameters (nlp="expr", branch_params=True)
and the Ohm's-law kernel with derivatives (hessian=True).  Both at the point a short Line Search asm_slp_run of the kernel form reaches,
on the working set of its multipliers, for the function phi = the sum of the first eight free p-flows + the multiplier of the middle
working row (gx, gl: unit entries; a seeded dense gradient is not a function of the solution at such a point - along a random direction
in all variables the KKT system of a 6-LP point is singular to working precision); --kkt-form (sparse) is the form of every solve.
Two handles in one process; the forms alternate call by call (block, expr, block, ...), so that both see the same clocks.  Timed, after a
warm-up call, on the host clock, every call ending with its results on the host; all repeats are printed, with median and spread
(max - min):
    adjoint        asm_solution_adjoint                                  --reps (9) repeats
    sens_one       asm_solution_sensitivity along one unit direction       --reps repeats (the size of one single-column solve)
    cross_t        asm_eval_data_cross_t alone                            --reps repeats
    cross          asm_eval_data_cross alone                              --reps repeats
    forward        the whole forward route, all constants                 --fwd-reps (2) repeats
Cross-check: per constant k, |adjoint[k] - forward[k]| against the bar of tests/test_adjoint_gpu.py's forward / reverse test,
1.51e-12 * (|gx|_1 |dx_k|_inf + |gl|_1 |dlam_k|_inf + |u_k|_1 |ax|_inf + |w_k|_1 |al|_inf); the largest ratio is reported.

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
LIMIT_S = 420
KKT_BAR = 1.51e-12


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def forward_route(opt, x, lam, rs, bs, nd, gx, gl, keep=None):
    """d phi / d dpar by the forward entries: 64 unit directions per asm_solution_sensitivity_multi call, contracted with (gx, gl)."""
    g = np.zeros(nd)
    statuses = set()
    for c0 in range(0, nd, 64):
        idx = np.arange(c0, min(c0 + 64, nd))
        DC = np.zeros((len(idx), nd))
        DC[np.arange(len(idx)), idx] = 1.0
        DX, DLAM, _, infos = opt.solution_sensitivity_multi(x, lam, rs, bs, DC)
        g[idx] = DX @ gx + DLAM @ gl
        statuses |= {int(i.status) for i in infos}
        if keep is not None:
            keep[0][idx], keep[1][idx] = np.abs(DX).max(axis=1), np.abs(DLAM).max(axis=1)
    return g, sorted(statuses)


def run_case(name, reps, fwd_reps, kkt_form):
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
        opts[form].set_kkt_form(kkt_form)
    run = opts["block"].slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    if rs.sum() > (bs == 0).sum():
        rs[np.nonzero(rs)[0][int((bs == 0).sum()):]] = 0
    rng = np.random.default_rng(9)
    mdl = fms["block"].acopf_model
    gx, gl = np.zeros(pr.n), np.zeros(pr.m)
    gx[[j for j in mdl.pf if bs[j] == 0][:8]] = 1.0
    gl[np.nonzero(rs == 1)[0][int(rs.sum()) // 2]] = 1.0
    vx, vl = rng.standard_normal(pr.n), rng.standard_normal(pr.m)
    out = dict(case=name, kkt_form=kkt_form, n=int(pr.n), m=int(pr.m), n_rows=int(rs.sum()), n_free=int((bs == 0).sum()), reps=reps, fwd_reps=fwd_reps)
    calls, res, nds = {}, {}, {}
    for form, opt in opts.items():
        nd = nds[form] = len(fms[form].nlp.device[2])
        e0 = np.zeros(nd)
        e0[0] = 1.0
        calls[form] = dict(adjoint=lambda o=opt: o.solution_adjoint(x, lam, rs, bs, gx, gl),
                           sens_one=lambda o=opt, d=e0: o.solution_sensitivity(x, lam, rs, bs, d),
                           cross_t=lambda o=opt: o.data_cross_t(x, lam, vx, vl), cross=lambda o=opt, d=e0: o.data_cross(x, lam, d),
                           forward=lambda o=opt, k=nd: forward_route(o, x, lam, rs, bs, k, gx, gl))
        res[form] = {k: dict(ms=[]) for k in calls[form]}
        res[form]["n_dpar"], res[form]["forward_calls"] = nd, -(-nd // 64)
    for key in calls["block"]:
        for form in calls:                     # warm-up
            got = calls[form][key]()
            if key == "adjoint":
                res[form][key].update(status=int(got[4].status), cg_iters=int(got[4].cg_iters))
            if key == "forward":
                res[form][key]["statuses"] = got[1]
        for _ in range(fwd_reps if key == "forward" else reps):      # the forms alternate
            for form in calls:
                ms, _ = timed(calls[form][key])
                res[form][key]["ms"].append(ms)
    for form, opt in opts.items():
        for key in calls[form]:
            r = res[form][key]
            r["median"] = float(np.median(r["ms"]))
            r["spread"] = float(max(r["ms"]) - min(r["ms"]))
        res[form]["forward_over_adjoint"] = res[form]["forward"]["median"] / res[form]["adjoint"]["median"]
        # the two gradients, constant by constant, against the bar of the forward / reverse test
        nd = nds[form]
        adj, _, ax, al, _ = calls[form]["adjoint"]()
        keep = (np.zeros(nd), np.zeros(nd))
        fwd, _ = forward_route(opt, x, lam, rs, bs, nd, gx, gl, keep)
        u1, w1 = np.zeros(nd), np.zeros(nd)
        for k in range(nd):
            dc = np.zeros(nd)
            dc[k] = 1.0
            u, w = opt.data_cross(x, lam, dc)
            u1[k], w1[k] = np.abs(u).sum(), np.abs(w).sum()
        bar = KKT_BAR * (np.abs(gx).sum() * keep[0] + np.abs(gl).sum() * keep[1] + u1 * np.abs(ax).max() + w1 * np.abs(al).max())
        live = bar > 0.0
        res[form]["max_abs_diff"] = float(np.abs(adj - fwd).max())
        res[form]["max_abs_gradient"] = float(np.abs(fwd).max())
        res[form]["max_diff_over_bar"] = float((np.abs(adj - fwd)[live] / bar[live]).max()) if live.any() else 0.0
        res[form]["diff_where_bar_is_zero"] = float(np.abs(adj - fwd)[~live].max()) if (~live).any() else 0.0
    out.update(res)
    for opt in opts.values():
        opt.close()
    return out


def main():
    reps, fwd_reps, form = arg("--reps", 9), arg("--fwd-reps", 2), arg("--kkt-form", "sparse")
    name = arg("--case", "case300")
    if "--child" in sys.argv:
        line = json.dumps(run_case(name, reps, fwd_reps, form))
        print(line)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(line + "\n")
        return 0
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", "--case", name, "--reps", str(reps), "--fwd-reps", str(fwd_reps),
           "--kkt-form", form]
    if "--out" in sys.argv:
        cmd += ["--out", arg("--out", "")]
    rc = subprocess.run(cmd).returncode
    if rc != 0:                                # a fault, an abort or a time limit: nothing more is started on the device
        print("%s ended with status %d" % (name, rc))
    return rc


if __name__ == "__main__":
    sys.exit(main())
