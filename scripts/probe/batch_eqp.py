"""SLP-EQP over a scenario batch: asm_batch_slp_run_eqp on S load scenarios of the case118-sized and case300-sized expression ACOPF
(nlp="expr") against (loop) asm_slp_run_eqp on one fresh handle per scenario, one after the other in the same process and from the
batch's basis columns - the comparator for time - and (tr) asm_batch_slp_run_tr on the same scenarios - the comparator for convergence.
Set-up (handles, batches, evaluators) is outside the clock; the clock is the host's around calls that end with their results on the
host.  One warm-up of every path at the timed shape (--warm a,b: of these only; the batch always), then --reps (default 3) rounds in
ABBA order (--order, default batch,loop,loop,batch,tr); every timed call reports its time on stderr as it ends.  Per path: wall time (median, min, max), converged count, iterations, LP solves, the summed eqp_counts and what the launch merging
did during one call (asm_batch_stats: ops, launches, rounds, emit_ms, wait_ms).  Also the device memory the first SLP-EQP call of a
batch takes per slot (hipMemGetInfo around it).  Prints one JSON line per (case, S); --out FILE appends them there.
--cases a,b (default case118,case300); --scenarios a,b (default 16,64); --max-iter K (default 200); --paths batch,loop,tr (default all:
with ASM_BATCH_VERBOSE=1 and --paths batch the per-kernel merge table on stderr is the SLP-EQP entry's alone); --load S."""
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import activesetmethods_amd as A  # noqa: E402
from activesetmethods_amd import _lib, acopf, batch  # noqa: E402

LOADS = {"case118": 1.0, "case300": 0.5}
STAT_KEYS = ("ops", "launches", "rounds", "emit_ms", "wait_ms")


def arg(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


def free_bytes():
    """Free device memory (hipMemGetInfo), None where the runtime library cannot be reached."""
    try:
        hip = ctypes.CDLL("libamdhip64.so")
        free, total = ctypes.c_size_t(0), ctypes.c_size_t(0)
        return int(free.value) if hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0 else None
    except OSError:
        return None


def summary(runs):
    out = dict(converged=sum(1 for r in runs if r.ret == 0), iterations=sum(r.iter for r in runs), lp_solves=sum(r.lp_solves for r in runs),
               iter_min=min(r.iter for r in runs), iter_max=max(r.iter for r in runs))
    if runs[0].eqp_counts is not None:
        out["eqp_counts"] = {k: sum(r.eqp_counts[k] for r in runs) for k in runs[0].eqp_counts}
    return out


def same_bits(a, b):
    return all(x.ret == y.ret and x.iter == y.iter and np.array_equal(x.x, y.x) and np.array_equal(x.lam, y.lam) and x.eqp_counts == y.eqp_counts
               for x, y in zip(a, b))


def main():
    reps, max_iter = arg("--reps", 3), arg("--max-iter", 200)
    which = arg("--paths", "batch,loop,tr").split(",")
    order, warm = arg("--order", "batch,loop,loop,batch,tr").split(","), arg("--warm", "batch,loop,tr").split(",")
    for case in arg("--cases", "case118,case300").split(","):
        load = arg("--load", LOADS.get(case, 1.0))
        base = acopf.synthetic_case(case, 1, load)
        for S in [int(v) for v in arg("--scenarios", "16,64").split(",")]:
            prs = [acopf.function_model(acopf.scenario_case(base, s), nlp="expr").to_problem("%s-sized scenario %d" % (case, s)) for s in range(S)]
            stack = tuple(np.stack([getattr(p, k) for p in prs]) for k in ("g_L", "g_U", "x_L", "x_U", "x0"))
            pars = {"eqp": A.Parameters(algorithm="SLP-EQP", max_iter=max_iter, device_eval=True),
                    "tr": A.Parameters(algorithm="Trust Region", max_iter=max_iter, device_eval=True)}
            hb = batch.HipBatch(prs[0], S)
            hb_tr = batch.HipBatch(prs[0], S) if "tr" in which else None
            stats = {}

            def run_batch(b=hb, par=pars["eqp"], key="batch"):
                s0 = b.stats()
                t0 = time.perf_counter()
                runs = b.slp_run(*stack, par)
                ms = 1e3 * (time.perf_counter() - t0)
                s1 = b.stats()
                stats[key] = {k: s1[k] - s0[k] for k in STAT_KEYS}
                return ms, runs

            def run_loop():
                ms, runs = 0.0, []
                for pr in prs:          # a fresh handle per scenario, set up outside the clock
                    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
                    opt.eval_setup(pr.function_model)
                    assert _lib.load().asm_sublp_set_ns_basis(opt._h, _lib.i32ptr(J), len(J)) == 0
                    t0 = time.perf_counter()
                    runs.append(opt.slp_run(pr.x0, pars["eqp"]))
                    ms += 1e3 * (time.perf_counter() - t0)
                    opt.close()
                return ms, runs

            def progress(fn, key):
                def run():
                    out = fn()
                    print("[batch_eqp] %s S=%d %s: %.0f ms" % (case, S, key, out[0]), file=sys.stderr, flush=True)
                    return out
                return run

            paths = {"batch": progress(run_batch, "batch"), "loop": progress(run_loop, "loop"),
                     "tr": progress(lambda: run_batch(hb_tr, pars["tr"], "tr"), "tr")}
            # warm-up at the timed shape; the batch's first SLP-EQP call also makes the slots' KKT buffers (two Trust-Region LPs per slot
            # first: what the LP solver makes at its first solves is not theirs)
            hb.slp_run(*stack, pars["tr"], max_lp_solves=2)
            f0 = free_bytes()
            _, last_batch = paths["batch"]()
            f1 = free_bytes()
            J = np.ascontiguousarray(hb.ns_basis(), np.int32)
            for k in which:
                if k != "batch" and k in warm:
                    paths[k]()
            ms, last = {k: [] for k in which}, {"batch": last_batch}
            for _ in range(reps):
                for k in order:
                    if k in which:
                        t, last[k] = paths[k]()
                        ms[k].append(t)
            out = dict(case=case, load=load, scenarios=S, n=prs[0].n, m=prs[0].m, max_iter=max_iter, groups=hb.groups, reps={k: len(v) for k, v in ms.items()},
                       kkt_mib_per_slot=(f0 - f1) / S / 2 ** 20 if f0 is not None and f1 is not None else None,
                       batch_equals_loop=same_bits(last["batch"], last["loop"]) if "loop" in which else None)
            for k in which:
                out[k] = dict(ms_median=float(np.median(ms[k])), ms_min=float(np.min(ms[k])), ms_max=float(np.max(ms[k])), **summary(last[k]))
                if k in stats:
                    out[k]["batch_stats"] = stats[k]
            hb.close()
            if hb_tr is not None:
                hb_tr.close()
            line = json.dumps(out)
            print(line, flush=True)
            if "--out" in sys.argv:
                with open(sys.argv[sys.argv.index("--out") + 1], "a") as f:
                    f.write(line + "\n")


if __name__ == "__main__":
    main()
