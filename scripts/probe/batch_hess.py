"""Hessians of the Lagrangian of 64 case300-sized line scenarios (expression ACOPF with branch parameters): one
asm_batch_hessian_lagrangian over all scenarios on a 64-slot batch against 64 separate per-handle evaluators, each set up with its
scenario's model and called once.  Both paths are timed on the host clock around calls that end with their results on the host, with
set-up (the first call after the evaluator set-up: lists and workspaces are made) and without (later calls), alternating in ABBA order.
Also the device memory of the Hessian lists (shared by the slots of a batch, private to a handle) and of one workspace, from the counts
of the host twin.  Prints one JSON line; --out FILE also writes it there; --scenarios N (default 64), --case NAME (default case300)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import acopf, batch  # noqa: E402


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def main():
    S, case = arg("--scenarios", 64), arg("--case", "case300")
    first_reps, steady_reps = arg("--first-reps", 2), arg("--reps", 20)
    base = acopf.synthetic_case(case, 1, 0.5)
    fms = [acopf.function_model(acopf.line_scenario_case(base, s), nlp="expr", branch_params=True) for s in range(S)]
    prs = [fm.to_problem("%s-sized line scenario %d" % (case, s)) for s, fm in enumerate(fms)]
    pr, n, m = prs[0], prs[0].n, prs[0].m
    rng = np.random.default_rng(1)
    X = np.stack([p.x0 for p in prs]) + 0.01 * rng.standard_normal((S, n))
    L = rng.standard_normal((S, m))

    hb = batch.HipBatch(pr, S)
    data = hb.scenario_data(prs)
    opts = []
    for p in prs:
        o = A.HipSubOptimizer(A.QpData(np.zeros(n), 0.0, np.zeros(p.nnz), np.zeros(m), p.g_L, p.g_U, p.x_L, p.x_U), p.j_row, p.j_col)
        opts.append(o)

    def fresh_batch():                  # evaluator set-up again: the next Hessian call builds the lists and the workspaces
        hb.setup(pr)
        hb.set_scenario_data(data)

    def fresh_loop():
        for o, fm in zip(opts, fms):
            o.eval_setup(fm)

    def call_batch():
        return hb.eval_hessian_lagrangian(X, 1.0, L)

    def call_loop():
        return np.stack([o.eval_hessian_lagrangian(X[s], 1.0, L[s]) for s, o in enumerate(opts)])

    def timed(fn):
        t0 = time.perf_counter()
        out = fn()
        return 1e3 * (time.perf_counter() - t0), out

    paths = {"batch": (fresh_batch, call_batch), "loop": (fresh_loop, call_loop)}
    fresh_batch()
    fresh_loop()
    for k in paths:                     # code objects, pinned staging, the scheduler's blobs: not part of either timing
        paths[k][1]()
    first = {k: [] for k in paths}
    for _ in range(first_reps):
        for k in ("batch", "loop", "loop", "batch"):
            paths[k][0]()
            first[k].append(timed(paths[k][1])[0])
    steady = {k: [] for k in paths}
    res = {}
    for _ in range(steady_reps):
        for k in ("batch", "loop", "loop", "batch"):
            t, res[k] = timed(paths[k][1])
            steady[k].append(t)
    same = bool(np.array_equal(res["batch"], res["loop"]))
    st0 = hb.stats()
    call_batch()
    st1 = hb.stats()
    hb.close()
    for o in opts:
        o.close()

    H = fms[0].nlp._hess_prepare()
    sweep = H["sweep"]
    nnz = len(fms[0].hessian_lagrangian_structure())
    nblk, nocc, Sd, wnodes = len(H["rows"]), len(H["othread"]), int(sweep.nr), int(sweep.lens.sum())
    nfn = nnz - nblk
    offdiag = sum(1 for r, c in fms[0].hessian_lagrangian_structure() if r != c)
    lists = 8 * (2 * nfn + (nblk + 1) + nocc + (n + 1) + 2 * (nnz + offdiag) + 3 * Sd + (Sd + 1) + nocc)
    slot = 8 * (4 * wnodes + nocc + m + 2 * n + nnz)
    out = dict(case=case, scenarios=S, n=n, m=m, hess_nnz=nnz, seed_threads=Sd, workspace_nodes=wnodes, occurrences=nocc,
               results_bit_identical=same, groups=hb.groups,
               lists_kib=lists / 1024.0, per_slot_kib=slot / 1024.0,
               batch_total_mib=(lists + S * slot) / 2 ** 20, loop_total_mib=S * (lists + slot) / 2 ** 20,
               ops_per_call=int(st1["ops"] - st0["ops"]), launches_per_call=int(st1["launches"] - st0["launches"]),
               rounds_per_call=int(st1["rounds"] - st0["rounds"]))
    for k in paths:
        out[k + "_first_ms"] = [round(t, 3) for t in first[k]]
        out[k + "_first_ms_median"] = float(np.median(first[k]))
        out[k + "_ms_median"] = float(np.median(steady[k]))
        out[k + "_ms_p10"] = float(np.percentile(steady[k], 10))
        out[k + "_ms_p90"] = float(np.percentile(steady[k], 90))
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
