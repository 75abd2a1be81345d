"""The static row order of the sparse KKT form (asm_kkt_set_order, asm_batch_kkt_set_form), measured.  Two parts, --part handle,batch
(default both); set-up (handles, batches, evaluators, models) is outside the clock, the clock is the host's around calls that end with
their results on the host, every path is warmed up once at the timed shape, the paths alternate call by call, and every repeat is kept:
median and spread (max - min) are printed beside them.

handle: expression ACOPFs of --cases (default case118,case300,case1354pegase; load scale 0.5), one handle per case in the sparse form, at
  the point a short Line Search asm_slp_run reaches, on the working set of its multipliers: asm_kkt_step at radius 0.4 in the working-set
  order against the static order, with the order cache (the same row_state again) and without it (two row_states that differ in one row
  take turns, so every call orders anew).  Per order: band, n_pairs, order_ms and the step's milliseconds.
batch: --scenarios (default 64) load scenarios of the case118-sized expression ACOPF (load scale 1.0, scripts/probe/batch_eqp.py's
  workload) through asm_batch_slp_run_eqp, a batch in the dense form against a batch in the sparse form and static order, alternating.
  Per form: seconds, converged count, iterations, summed trial counts, ops / launches / rounds of the launch merging, the bytes a slot
  holds (asm_kkt_form_info through asm_batch_handle).  With ASM_BATCH_VERBOSE=1 each batch prints its per-kernel merge table on stderr
  when it is released: the dense batch first, then the sparse one.
--reps N (default 5 for handle, 3 for batch); --max-iter K (default 200).  Prints one JSON line per case or batch; --out FILE appends
them there."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import _lib, acopf, batch, sensitivity  # noqa: E402

ORDERS = ("working-set", "static")


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def emit(out):
    line = json.dumps(out)
    print(line, flush=True)
    if "--out" in sys.argv:
        with open(arg("--out", ""), "a") as f:
            f.write(line + "\n")


def stat(v):
    return dict(all=[float(x) for x in v], median=float(np.median(v)), spread=float(max(v) - min(v)))


def handle_case(name, reps):
    fm = acopf.function_model(acopf.synthetic_case(name, 1, 0.5), nlp="expr")
    pr = fm.to_problem(name)
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    run = opt.slp_run(pr.x0, A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True), 6)
    x, lam = run.x, run.lam
    rs, bs = sensitivity.working_set(pr, x, lam, run.mult_x_U, run.mult_x_L, tol=1e-6)
    if rs.sum() > (bs == 0).sum():
        rs[np.nonzero(rs)[0][int((bs == 0).sum()):]] = 0
    other = rs.copy()
    other[np.nonzero(rs)[0][-1]] = 0                       # the second row_state of the runs without the cache
    _, df, E = opt.eval_functions(x)
    rw = np.where(rs == 1, E - np.where(np.isfinite(pr.g_L), pr.g_L, pr.g_U), 0.0)
    opt.set_kkt_form("sparse")
    out = dict(part="handle", case=name, n=int(pr.n), m=int(pr.m), n_rows=int(rs.sum()), n_free=int((bs == 0).sum()), reps=reps)
    res = {o: dict(cached=dict(step_ms=[], order_ms=[]), cold=dict(step_ms=[], order_ms=[])) for o in ORDERS}

    def step(order, rows, into=None):
        opt.set_kkt_order(order)
        t0 = time.perf_counter()
        got = opt.kkt_step(x, lam, rows, bs, df, rw, 0.4)
        ms = 1e3 * (time.perf_counter() - t0)
        fi = opt.kkt_form_info()
        if into is not None:
            into["step_ms"].append(ms)
            into["order_ms"].append(float(fi.order_ms))
        return got, fi
    for o in ORDERS:                                       # warm-up: buffers, and the figures of the order
        got, fi = step(o, rs)
        res[o].update(band=int(fi.band), n_pairs=int(fi.n_pairs), form_used=int(fi.form_used), status=int(got[3].status), cg_iters=int(got[3].cg_iters))
        res[o]["dx"] = got[0]
    for k in range(reps):                                  # without the cache: the row_states take turns, the orders alternate
        for o in ORDERS:
            _, fi = step(o, other if k % 2 == 0 else rs, res[o]["cold"])
            assert fi.order_reused == 0
    for k in range(reps):                                  # with it
        for o in ORDERS:
            step(o, rs)
            _, fi = step(o, rs, res[o]["cached"])
            assert fi.order_reused == 1
    dxs = [res[o].pop("dx") for o in ORDERS]
    out["max_rel_diff_dx"] = float(np.abs(dxs[0] - dxs[1]).max() / max(1.0, np.abs(dxs[0]).max()))
    oi = opt.kkt_order_info()
    out.update(all_band=int(oi.all_band), all_pairs=int(oi.all_pairs))
    for o in ORDERS:
        for kind in ("cached", "cold"):
            res[o][kind] = {k: stat(v) for k, v in res[o][kind].items()}
    out.update(res)
    opt.close()
    emit(out)


def batch_part(S, reps, max_iter):
    base = acopf.synthetic_case("case118", 1, 1.0)
    prs = [acopf.function_model(acopf.scenario_case(base, s), nlp="expr").to_problem("case118-sized scenario %d" % s) for s in range(S)]
    stack = tuple(np.stack([getattr(p, k) for p in prs]) for k in ("g_L", "g_U", "x_L", "x_U", "x0"))
    forms = {"dense": ("dense", "working-set"), "sparse-static": ("sparse", "static")}
    pars = {k: A.Parameters(algorithm="SLP-EQP", max_iter=max_iter, device_eval=True, kkt_form=f, kkt_order=o) for k, (f, o) in forms.items()}
    hbs = {k: batch.HipBatch(prs[0], S) for k in forms}
    out = dict(part="batch", case="case118", load=1.0, scenarios=S, n=prs[0].n, m=prs[0].m, max_iter=max_iter, groups=hbs["dense"].groups)
    res = {k: dict(s=[]) for k in forms}

    def run(k, keep=True):
        s0 = hbs[k].stats()
        t0 = time.perf_counter()
        runs = hbs[k].slp_run(*stack, pars[k])
        sec = time.perf_counter() - t0
        s1 = hbs[k].stats()
        print("[batch_eqp_sparse] S=%d %s: %.2f s" % (S, k, sec), file=sys.stderr, flush=True)
        if keep:
            res[k]["s"].append(sec)
        res[k].update(converged=sum(1 for r in runs if r.ret == 0), iterations=sum(r.iter for r in runs),
                      eqp_counts={c: sum(r.eqp_counts[c] for r in runs) for c in runs[0].eqp_counts},
                      batch_stats={c: s1[c] - s0[c] for c in ("ops", "launches", "rounds", "emit_ms", "wait_ms")})
    for k in forms:
        run(k, keep=False)
    for _ in range(reps):
        for k in forms:
            run(k)
    lib = _lib.load()
    for k in forms:
        fi = _lib.KktFormInfo()
        assert lib.asm_kkt_form_info(lib.asm_batch_handle(hbs[k]._b, 0), C.byref(fi)) == 0
        res[k].update(form_used=int(fi.form_used), dense_bytes_per_slot=int(fi.dense_bytes), sparse_bytes_per_slot=int(fi.sparse_bytes), s=stat(res[k]["s"]))
        hbs[k].close()                                     # (ASM_BATCH_VERBOSE=1: the merge table of this form)
    out.update(res)
    emit(out)


def main():
    parts = arg("--part", "handle,batch").split(",")
    if "handle" in parts:
        for name in arg("--cases", "case118,case300,case1354pegase").split(","):
            handle_case(name, arg("--reps", 5))
    if "batch" in parts:
        batch_part(arg("--scenarios", 64), arg("--reps", 3), arg("--max-iter", 200))


if __name__ == "__main__":
    main()
