"""Launches per conjugate-gradient round of the KKT entries, from a rocprofv3 --kernel-trace CSV.
  python scripts/probe/kkt_round_launches.py run ENTRY     one call of ENTRY (solve, solve_multi, step, step_multi) on the (96, 10, 65)
                                                          constructed QP, 5 columns for the multi entries - the program to put after
                                                          `rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME --`
  python scripts/probe/kkt_round_launches.py count CSV    the dispatches from one k_kktm_cg_dir to the next, as a histogram: the most
                                                          frequent length is the round (the first and last segments hold the set-up and
                                                          the finish), and the kernels of one such round by name"""
import collections
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def run(entry):
    import numpy as np
    import activesetmethods_amd as A
    from tests.test_sensitivity_cpu import kkt_instance
    from tests.test_sensitivity_multi_cpu import multi_columns
    inst = kkt_instance(96, 10, 65)
    fm, x, lam, rs, bs, ru, rw = inst
    RU, RW = multi_columns(inst, 5)
    pr = fm.to_problem()
    opt = A.HipSubOptimizer(A.QpData(np.zeros(pr.n), 0.0, np.zeros(pr.nnz), np.zeros(pr.m), pr.g_L, pr.g_U, pr.x_L, pr.x_U), pr.j_row, pr.j_col)
    opt.eval_setup(fm)
    big = 1e3                                                # a radius no column reaches: every round is a full one
    out = {"solve": lambda: opt.kkt_solve(x, lam, rs, bs, ru, rw), "solve_multi": lambda: opt.kkt_solve_multi(x, lam, rs, bs, RU, RW),
           "step": lambda: opt.kkt_step(x, lam, rs, bs, ru, rw, big), "step_multi": lambda: opt.kkt_step_multi(x, lam, rs, bs, RU, RW, np.full(5, big))}[entry]()
    info = out[3] if entry in ("solve", "step") else out[3][0]
    print(entry, "cg_iters", info.cg_iters)
    opt.close()


def count(path):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"].split("(")[0] for r in rows]
    marks = [i for i, nm in enumerate(names) if "k_kktm_cg_dir" in nm]
    lengths = [b - a for a, b in zip(marks, marks[1:])]
    hist = collections.Counter(lengths)
    print("dispatches %d, k_kktm_cg_dir %d, launches from one k_kktm_cg_dir to the next: %r" % (len(names), len(marks), sorted(hist.items())))
    if hist:
        mode = hist.most_common(1)[0][0]
        a = next(a for a, b in zip(marks, marks[1:]) if b - a == mode)
        print("a round of %d launches: %s" % (mode, ", ".join(nm.split("<")[0][-28:] for nm in names[a + 1:a + mode + 1])))


if __name__ == "__main__":
    run(sys.argv[2]) if sys.argv[1] == "run" else count(sys.argv[2])
