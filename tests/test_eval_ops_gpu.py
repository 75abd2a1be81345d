"""The stream operations of the derivative entries, per NLP block family (csrc/asm_hip.hip, "NLP block kinds"): a 2-slot batch with 2
scenarios of one small instance of each family - the Ohm's-law kernel with derivatives on the 3-bus grid, the dense quadratic kernel
with derivatives on (n, m) = (5, 3), an expression tape with constants, one without - counts the operations its slots record
(asm_batch_get_stats: ops) in one call of each entry, first call and repeat.  Every launch, copy and fill of an entry is one operation,
so a count that moves is a path that gained or lost one."""
import numpy as np
import pytest

from activesetmethods_amd import acopf, batch, problems
from activesetmethods_amd.nlexpr import ExprBlock, variables
from tests.test_nlexpr_cpu import _model
from tests.test_ohm_hess_cpu import grid
from tests.test_sensitivity_gpu import hs071_param_model

pytestmark = pytest.mark.gpu

# ops of (first call, repeat) per entry, in the call order of ENTRIES on a fresh batch.  These are the counts of the commit before the
# block kinds got one home (the parent of the commit that added this test), recorded by running this test on that build.
PARENT_OPS = {
    'grid3 ohm (kind 4)': {'data_gradient': (8, 8), 'hessian_lagrangian': (22, 12), 'hessian_product': (16, 16), 'solution_sensitivity': (221, 221), 'solution_adjoint': (210, 210)},
    'dense 5x3 (kind 5)': {'data_gradient': (8, 8), 'hessian_lagrangian': (18, 10), 'hessian_product': (14, 14), 'solution_sensitivity': (262, 262), 'solution_adjoint': (266, 266)},
    'tape with constants': {'data_gradient': (10, 10), 'hessian_lagrangian': (28, 10), 'hessian_product': (14, 14), 'solution_sensitivity': (218, 218), 'solution_adjoint': (212, 212)},
    'tape without constants': {'data_gradient': (0, 0), 'hessian_lagrangian': (28, 10), 'hessian_product': (14, 14), 'solution_sensitivity': (138, 138), 'solution_adjoint': (168, 168)},
}
ENTRIES = ("data_gradient", "hessian_lagrangian", "hessian_product", "solution_sensitivity", "solution_adjoint")


def _tape_without_constants():
    x = variables(2)
    return _model(ExprBlock([(x[0] * x[1], 0.0, 0.0)], objective=x[0] * x[0], n=2), 2)


MODELS = {"grid3 ohm (kind 4)": lambda: acopf.function_model(grid("grid3"), hessian=True),
          "dense 5x3 (kind 5)": lambda: problems.synthetic_dense_function_model(5, 3, hessian=True),
          "tape with constants": hs071_param_model,
          "tape without constants": _tape_without_constants}


@pytest.mark.parametrize("name", list(MODELS))
def test_ops_of_one_call_of_each_entry(name):
    fm = MODELS[name]()
    pr = fm.to_problem(name)
    n, m, S = pr.n, pr.m, 2
    hb = batch.HipBatch(pr, 2)
    nd = hb.n_dpar
    rng = np.random.default_rng(7)
    X = np.stack([pr.x0 + 0.01 * (s + 1) * rng.uniform(-1.0, 1.0, n) for s in range(S)])
    L = rng.standard_normal((S, m))
    # the equality rows and no bound: a valid working set at any point (none where the rows outnumber the variables)
    eq = (pr.g_L == pr.g_U).astype(np.int32)
    rs = np.stack([eq if eq.sum() <= n else np.zeros(m, np.int32)] * S)
    bs = np.zeros((S, n), np.int32)
    V, DC = rng.standard_normal((S, n)), rng.standard_normal((3, nd))
    GX, GL = rng.standard_normal((S, 2, n)), rng.standard_normal((S, 2, m))
    calls = {"data_gradient": lambda: hb.data_gradient(X, L),
             "hessian_lagrangian": lambda: hb.eval_hessian_lagrangian(X, 1.0, L),
             "hessian_product": lambda: hb.hessian_product(X, 1.0, L, V),
             "solution_sensitivity": lambda: hb.solution_sensitivity_multi(X, L, rs, bs, DC),
             "solution_adjoint": lambda: hb.solution_adjoint(X, L, rs, bs, GX, GL)}
    hb.hessian_structure()                                               # (eval_hessian_lagrangian asks for it: outside the counts)
    got = {}
    for entry in ENTRIES:
        counts = []
        for _ in range(2):
            before = hb.stats()["ops"]
            calls[entry]()
            counts.append(hb.stats()["ops"] - before)
        got[entry] = tuple(counts)
    hb.close()
    print("%r: %r," % (name, got))
    assert got == PARENT_OPS[name]
