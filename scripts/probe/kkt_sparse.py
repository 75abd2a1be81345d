"""The two forms of the KKT solve (asm_kkt_set_form) side by side on expression ACOPFs of three sizes: case118-, case300- and
case1354pegase-sized (load scale 0.5), each at the point a short Line Search asm_slp_run reaches, on the working set of its multipliers.
One handle per case, one process; the forms alternate call by call (sparse, dense, sparse, ...), so that both see the same clocks.  The
dense form is the comparator: it is the code path the library had before the sparse form.  Per case and form: one asm_kkt_step and a
64-column asm_kkt_step_multi (a radius ladder of the same right-hand side) from the same point at the trial radius of SLP-EQP (0.4:
the step ends on the boundary after a round or two, the call is its set-up), and both again without a radius (the iteration runs to
its end) - warm-up, then --reps (5) repeats on the host clock, every call ending with its results on the host; all repeats are printed,
with median and spread (max - min).  Also: band, n_pairs, dense_bytes / sparse_bytes, the conjugate-gradient rounds of the calls and
milliseconds per round (the difference of the two kinds of call over the difference of their rounds), the host time of the row order
without the cache (the first call on a row_state) and with it.

This file is the parent; every case runs in a child process of its own under `timeout` (--case NAME runs one case in this process), so
that a case that takes too long ends alone.  --skip-dense-above N: the dense form of a case with more than N variables is set up and
timed ONCE (no warm-up, no repeats; default: every case is repeated).  Prints one JSON line per case; --out FILE appends them there."""
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
CASES = ("case118", "case300", "case1354pegase")
LIMIT_S = {"case118": 120, "case300": 180, "case1354pegase": 420}


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def run_case(name, reps, dense_once_above):
    import activesetmethods_amd as A
    from activesetmethods_amd import acopf, sensitivity
    fm = acopf.function_model(acopf.synthetic_case(name, 1, 0.5), nlp="expr")
    pr = fm.to_problem(name)
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    if rs.sum() > (bs == 0).sum():
        rs[np.nonzero(rs)[0][int((bs == 0).sum()):]] = 0
    f, df, E = opt.eval_functions(x)
    rw = np.where(rs == 1, E - np.where(np.isfinite(pr.g_L), pr.g_L, pr.g_U), 0.0)
    out = dict(case=name, n=int(pr.n), m=int(pr.m), nnz=int(pr.nnz), n_rows=int(rs.sum()), n_free=int((bs == 0).sum()), reps=reps)
    dense_once = pr.n > dense_once_above
    radius = 0.4
    radii = radius * np.linspace(0.05, 1.5, 64)
    RU, RW = np.tile(df, (64, 1)), np.tile(rw, (64, 1))
    far = np.full(64, np.inf)
    calls = dict(step=lambda: opt.kkt_step(x, lam, rs, bs, df, rw, radius), step_multi_64=lambda: opt.kkt_step_multi(x, lam, rs, bs, RU, RW, radii),
                 step_inf=lambda: opt.kkt_step(x, lam, rs, bs, df, rw, np.inf), step_multi_64_inf=lambda: opt.kkt_step_multi(x, lam, rs, bs, RU, RW, far))
    res = {form: {k: dict(ms=[]) for k in calls} for form in ("sparse", "dense")}
    # the first call of each form: buffers, and for the sparse form the row order without the cache
    for form in ("sparse", "dense"):
        opt.set_kkt_form(form)
        ms, got = timed(calls["step"])
        fi = opt.kkt_form_info()
        res[form]["first_call_ms"] = ms
        res[form].update(form_used=int(fi.form_used), band=int(fi.band), n_pairs=int(fi.n_pairs), order_ms_no_cache=float(fi.order_ms),
                         status=int(got[3].status), cg_iters=int(got[3].cg_iters), boundary=int(got[3].boundary), dropped=int(got[3].dropped_pivots))
    if dense_once:
        res["dense"]["timed_once"] = True
        opt.set_kkt_form("dense")
        ms, got = timed(calls["step_multi_64"])
        res["dense"]["step_multi_64"]["ms"].append(ms)
        res["dense"]["step_multi_64"]["rounds"] = int(max(i.cg_iters for i in got[3]))
        res["dense"]["step"]["ms"].append(res["dense"]["first_call_ms"])
        res["dense"]["step"]["rounds"] = res["dense"]["cg_iters"]
    forms = ("sparse",) if dense_once else ("sparse", "dense")
    for key, fn in calls.items():
        for form in forms:                     # warm-up
            opt.set_kkt_form(form)
            got = fn()
            infos = got[3] if isinstance(got[3], list) else [got[3]]
            res[form][key]["rounds"] = int(max(i.cg_iters for i in infos))
        for _ in range(reps):                  # the forms alternate
            for form in forms:
                opt.set_kkt_form(form)
                ms, _ = timed(fn)
                res[form][key]["ms"].append(ms)
                if form == "sparse":
                    fi = opt.kkt_form_info()
                    res[form].setdefault("order_ms_cached", []).append(float(fi.order_ms))
                    res[form]["order_reused"] = int(fi.order_reused)
    for form in ("sparse", "dense"):
        for key in calls:
            r = res[form][key]
            r["median"] = float(np.median(r["ms"]))
            r["spread"] = float(max(r["ms"]) - min(r["ms"]))
        # a conjugate-gradient round: what the calls without a radius cost beyond the calls that stop after the trial radius's rounds
        for short, full in (("step", "step_inf"), ("step_multi_64", "step_multi_64_inf")):
            a, b = res[form][short], res[form][full]
            if b.get("rounds", 0) > a.get("rounds", 0):
                b["ms_per_round"] = (b["median"] - a["median"]) / (b["rounds"] - a["rounds"])
    fi = opt.kkt_form_info()
    out.update(res, dense_bytes=int(fi.dense_bytes), sparse_bytes=int(fi.sparse_bytes))
    if not dense_once:                         # the two forms' answers, for the record
        opt.set_kkt_form("sparse")
        sp = calls["step"]()
        opt.set_kkt_form("dense")
        de = calls["step"]()
        out["max_rel_diff_dx"] = float(np.abs(sp[0] - de[0]).max() / max(1.0, np.abs(de[0]).max()))
    opt.close()
    return out


def main():
    reps, above = arg("--reps", 5), arg("--skip-dense-above", 10 ** 9)
    if "--case" in sys.argv:
        line = json.dumps(run_case(arg("--case", ""), reps, above))
        print(line)
        if "--out" in sys.argv:
            with open(arg("--out", ""), "a") as f:
                f.write(line + "\n")
        return 0
    names = [c for c in CASES if c in sys.argv] or list(CASES)
    for name in names:
        cmd = ["timeout", "-k", "10", str(LIMIT_S[name]), sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(reps), "--skip-dense-above", str(above)]
        if "--out" in sys.argv:
            cmd += ["--out", arg("--out", "")]
        rc = subprocess.run(cmd).returncode
        if rc != 0:                            # a fault, an abort or a time limit: nothing more is started on the device
            print("%s ended with status %d: stopping" % (name, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
