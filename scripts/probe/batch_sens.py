"""Solution and bound sensitivities of 64 case300-sized line scenarios (expression ACOPF with branch parameters) at the points of a batch
SLP-EQP run: asm_batch_solution_sensitivity / asm_batch_bound_sensitivity over all scenarios on a 64-slot batch against a loop of
asm_solution_sensitivity_multi / asm_kkt_solve_multi over 64 per-handle evaluators, each set up with its scenario's model - the per-handle
entries are what a user had before the batch entries.  8 and 64 unit data directions and 8 bound rows, in the dense form and in the
sparse form with the static row order.  Both paths are timed on the host clock around calls that end with their results on the host, with
set-up (the first call after the evaluator set-up: lists, work areas and workspaces are made) and without (later calls), alternating in
ABBA order.  Also the batch's operations per launch and the bytes of a slot's 64-column work area.  Prints one JSON line; --out FILE also
writes it there; --scenarios N (default 64), --case NAME (default case300), --reps R warm repetitions (default 3), --max-lp K LP solves
per scenario of the run that makes the points (default 0: until it ends)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import _lib, acopf, batch, sensitivity  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def up(v, q):
    return (int(v) + q - 1) // q * q


def main():
    S, case, reps = arg("--scenarios", 64), arg("--case", "case300"), arg("--reps", 3)
    base = acopf.synthetic_case(case, 1, 0.5)
    fms = [acopf.function_model(acopf.line_scenario_case(base, s), nlp="expr", branch_params=True) for s in range(S)]
    prs = [fm.to_problem("%s-sized line scenario %d" % (case, s)) for s, fm in enumerate(fms)]
    pr, n, m = prs[0], prs[0].n, prs[0].m
    nd = len(fms[0].nlp.device[2])
    par = A.Parameters(algorithm="SLP-EQP", max_iter=60, device_eval=True)

    hb = batch.HipBatch(pr, S)
    data = hb.scenario_data(prs)
    stack = lambda k: np.stack([getattr(p, k) for p in prs])
    t0 = time.perf_counter()
    runs = hb.slp_run(stack("g_L"), stack("g_U"), stack("x_L"), stack("x_U"), stack("x0"), par, max_lp_solves=arg("--max-lp", 0), data=data)
    run_s = time.perf_counter() - t0
    rs, bs = batch.working_sets(prs, runs)
    replaced = 0
    for s in range(S):                  # a point whose active rows outnumber its free variables: the equality rows alone, no bound
        if rs[s].sum() > (bs[s] == 0).sum():
            rs[s], bs[s], replaced = (prs[s].g_L == prs[s].g_U).astype(np.int32), 0, replaced + 1
    X, L = np.stack([r.x for r in runs]), np.stack([r.lam for r in runs])
    rng = np.random.default_rng(1)
    cols = {8: np.sort(rng.choice(nd, 8, replace=False)), 64: np.sort(rng.choice(nd, 64, replace=False))}
    DC = {k: np.zeros((k, nd)) for k in cols}
    for k, idx in cols.items():
        DC[k][np.arange(k), idx] = 1.0
    eq = np.nonzero(pr.g_L[:fms[0].nlp_constraint_offset] == pr.g_U[:fms[0].nlp_constraint_offset])[0]
    rows = eq[-8:].astype(np.int32)     # eight balance rows: equalities, in every working set
    RU, RW = sensitivity.bound_rhs(m, n, rows)

    opts = [A.HipSubOptimizer(A.QpData(np.zeros(n), 0.0, np.zeros(p.nnz), np.zeros(m), p.g_L, p.g_U, p.x_L, p.x_U), p.j_row, p.j_col) for p in prs]
    order = {"dense": "working-set", "sparse": "static"}
    out = dict(case=case, scenarios=S, n=n, m=m, n_dpar=nd, groups=hb.groups, points_run_s=run_s, converged=sum(r.ret == 0 for r in runs),
               working_rows=[int(rs.sum(1).min()), int(rs.sum(1).max())], free_variables=[int((bs == 0).sum(1).min()), int((bs == 0).sum(1).max())],
               working_sets_replaced=replaced)
    ldn, Mp, ldT = up(n, 32), max(up(m, 16), 32), up(min(m, n), 32)
    out["work_area_bytes_per_slot"] = {"columns": 8 * 64 * (14 * ldn + 5 * ldT + Mp), "transposed_factor": 8 * ldT * ldT, "dense_only_AfT": 8 * ldn * ldT}

    def timed(fn):
        t0 = time.perf_counter()
        res = fn()
        return 1e3 * (time.perf_counter() - t0), res

    for form in ("dense", "sparse"):
        def fresh_batch():
            hb.setup(pr)
            hb.set_scenario_data(data)
            hb.set_kkt_form(form, order[form])

        def fresh_loop():
            for o, fm in zip(opts, fms):
                o.eval_setup(fm)
                o.set_kkt_form(form)
                o.set_kkt_order(order[form])
        calls = {}
        for k in cols:
            calls["data%d" % k] = (lambda k=k: hb.solution_sensitivity_multi(X, L, rs, bs, DC[k]),
                                   lambda k=k: [o.solution_sensitivity_multi(X[s], L[s], rs[s], bs[s], DC[k]) for s, o in enumerate(opts)])
        calls["bound8"] = (lambda: hb.bound_sensitivity(X, L, rs, bs, rows),
                           lambda: [o.kkt_solve_multi(X[s], L[s], rs[s], bs[s], RU, RW) for s, o in enumerate(opts)])
        fresh_batch()
        fresh_loop()
        res = {}
        for name, (cb, cl) in calls.items():
            fns = {"batch": cb, "loop": cl}
            for k in fns:               # code objects, pinned staging, the scheduler's blobs: not part of either timing
                fns[k]()
            warm = {"batch": [], "loop": []}
            got = {}
            for _ in range(reps):
                for k in ("batch", "loop", "loop", "batch"):
                    t, got[k] = timed(fns[k])
                    warm[k].append(t)
            st0 = hb.stats()
            cb()
            st1 = hb.stats()
            same = all(np.array_equal(got["batch"][q][s], got["loop"][s][q]) for s in range(S) for q in range(3))
            status = sorted({i.status for row in got["batch"][3] for i in row})
            iters = [i.cg_iters for row in got["batch"][3] for i in row]
            res[name] = dict(batch_ms=[round(t, 2) for t in warm["batch"]], loop_ms=[round(t, 2) for t in warm["loop"]],
                             batch_ms_median=float(np.median(warm["batch"])), loop_ms_median=float(np.median(warm["loop"])),
                             bit_identical=bool(same), statuses=status, cg_iters=[int(min(iters)), int(max(iters))],
                             ops=int(st1["ops"] - st0["ops"]), launches=int(st1["launches"] - st0["launches"]), rounds=int(st1["rounds"] - st0["rounds"]))
        first = {"batch": [], "loop": []}
        cb, cl = calls["data8"]
        for k in ("batch", "loop", "loop", "batch"):          # with the set-up: 8 data directions
            (fresh_batch if k == "batch" else fresh_loop)()
            first[k].append(round(timed(cb if k == "batch" else cl)[0], 2))
        res["data8_first_call_ms"] = first
        info = _lib.KktFormInfo()
        assert hb._lib.asm_kkt_form_info(hb._lib.asm_batch_handle(hb._b, 0), hb._C.byref(info)) == 0
        res["slot0"] = dict(form_used=int(info.form_used), dense_bytes=int(info.dense_bytes), sparse_bytes=int(info.sparse_bytes), band=int(info.band))
        out[form] = res
    hb.close()
    for o in opts:
        o.close()
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
