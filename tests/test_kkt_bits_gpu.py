"""The KKT solve returns the bits it returned before its single and multi drivers were merged: asm_kkt_solve, asm_kkt_solve_multi,
asm_solution_sensitivity and asm_solution_sensitivity_multi against outputs recorded on an MI355X (tests/golden/kkt_bits.npz).

The fixture was recorded once, by running this module as a script (python -m tests.test_kkt_bits_gpu OUT.npz) against a build of the
parent of the merging commit, kept apart from the tree under test as a git worktree outside the repository keeps it; the module uses
only Python API that parent has.  A change of
the toolchain (compiler, ROCm) is the only legitimate reason to record it again, and a new recording is taken from the parent of the
commit that makes that change - never from the code under test.

The cases are the smallest that cover |W| = 0, a vertex, one and two factor blocks (63 and 65 working rows around the 64-wide block),
more than one reduction workgroup (n = 200: ldn > 256), all four status codes and a chunk with a frozen column."""
import os
import sys

import numpy as np
import pytest

from tests.test_nlparams_gpu import _handle_for
from tests.test_sensitivity_cpu import KKT_SHAPES, kkt_instance
from tests.test_sensitivity_gpu import hs071_param_model
from tests.test_sensitivity_multi_cpu import multi_columns

pytestmark = pytest.mark.gpu
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kkt_bits.npz")
HS071_DC = np.array([[1.0, 0.0], [0.0, 1.0], [0.3, -0.2]])         # the directions of the hs071 tests


def _pack(outs):
    """[(dx, dlam, dz, info), ...] of single calls, or one (DX, DLAM, DZ, infos) of a multi call -> dict of arrays, a row per column."""
    if not isinstance(outs, list):
        outs = [(outs[0][c], outs[1][c], outs[2][c], outs[3][c]) for c in range(len(outs[3]))]
    return dict(dx=np.array([o[0] for o in outs]), dlam=np.array([o[1] for o in outs]), dz=np.array([o[2] for o in outs]),
                codes=np.array([[o[3].status, o[3].cg_iters, o[3].dropped_pivots] for o in outs], np.int64),
                res=np.array([[o[3].res_stat, o[3].res_feas] for o in outs]))


def _single(inst, **kw):
    fm, x, lam, rs, bs, ru, rw = inst
    opt = _handle_for(fm.to_problem(), fm)
    out = opt.kkt_solve(x, lam, rs, bs, ru, rw, **kw)
    opt.close()
    return _pack([out])


def _multi(cols):
    inst = kkt_instance(96, 10, 65)
    fm, x, lam, rs, bs = inst[:5]
    RU, RW = multi_columns(inst, 7)
    opt = _handle_for(fm.to_problem(), fm)
    out = opt.kkt_solve_multi(x, lam, rs, bs, np.ascontiguousarray(RU[cols]), np.ascontiguousarray(RW[cols]))
    opt.close()
    return _pack(out)


def _hs071(multi):
    """The closed working set of hs071's solution (both rows, x1 at its lower bound) at a fixed point near it: no SLP run."""
    fm = hs071_param_model()
    pr = fm.to_problem("hs071 rhs parameters")
    x = pr.x0 + np.array([0.0, -0.257, -1.1789, 0.3794])
    lam = np.array([0.55229, -0.16147])
    rs, bs = np.array([1, 1], np.int32), np.array([-1, 0, 0, 0], np.int32)
    opt = _handle_for(pr, fm)
    out = opt.solution_sensitivity_multi(x, lam, rs, bs, HS071_DC) if multi else [opt.solution_sensitivity(x, lam, rs, bs, dc) for dc in HS071_DC]
    opt.close()
    return _pack(out)


def _curvature():
    neg = np.full(8, 4.0)
    neg[2] = -50.0
    return _single(kkt_instance(8, 0, 2, seed=3, diag=neg))


CASES = {"single_n%d_B%d_W%d" % s: (lambda s=s: _single(kkt_instance(*s))) for s in KKT_SHAPES}
CASES.update({
    "single_curvature": _curvature,
    "single_duplicate_row": lambda: _single(kkt_instance(12, 2, 4, seed=4, duplicate_row=True)),
    "single_iteration_limit": lambda: _single(kkt_instance(200, 20, 130), max_iter=1, rtol=1e-12),
    "multi_7_columns": lambda: _multi(slice(0, 7)),
    "multi_column_3_alone": lambda: _multi(slice(3, 4)),
    "sensitivity_hs071": lambda: _hs071(False),
    "sensitivity_multi_hs071": lambda: _hs071(True),
})
FIELDS = ("dx", "dlam", "dz", "codes", "res")


@pytest.fixture(scope="module")
def recorded():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", sorted(CASES))
def test_same_bits_as_recorded(recorded, name):
    got = CASES[name]()
    want = {f: recorded[name + "." + f] for f in FIELDS}
    print("%s: (status, cg_iters, dropped_pivots) %r, residuals %r" % (name, got["codes"].tolist(), got["res"].tolist()))
    assert got["codes"].tolist() == want["codes"].tolist()                      # status, cg_iters, dropped_pivots
    for f in ("dx", "dlam", "dz", "res"):                                       # res: res_stat, res_feas
        assert got[f].shape == want[f].shape and np.array_equal(got[f], want[f]), (name, f, float(np.abs(got[f] - want[f]).max()))


def test_the_recorded_cases_cover_every_status_and_a_frozen_column(recorded):
    status = {int(s) for name in CASES for s in recorded[name + ".codes"][:, 0]}
    assert status == {0, 1, 2, 3}
    iters = recorded["multi_7_columns.codes"][:, 1]
    assert iters[1] == 0 and len(set(iters.tolist())) >= 2 and sorted(k.rsplit(".", 1)[0] for k in recorded if k.endswith(".dx")) == sorted(CASES)


if __name__ == "__main__":
    rec = {}
    for case in sorted(CASES):
        for field, v in CASES[case]().items():
            rec[case + "." + field] = v
        print(case, rec[case + ".codes"].tolist())
    np.savez_compressed(sys.argv[1], **rec)
    print("recorded %d arrays, %d bytes" % (len(rec), os.path.getsize(sys.argv[1])))
