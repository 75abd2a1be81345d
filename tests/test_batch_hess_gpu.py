"""The Hessian of the Lagrangian of a scenario batch (include/asm_hip.h: asm_batch_hessian_structure, asm_batch_hessian_lagrangian,
asm_batch_hessian_product) against the per-handle entries on fresh handles (bit for bit, every op) and the host twin (bit for bit on
arithmetic tapes, the parity bar with math-library ops): per-scenario data through the table and without one, more scenarios than
slots, launch merging, no interference with the SLP state, argument and state errors, batch.lagrangian_hessians."""
import ctypes as C
import functools

import numpy as np
import pytest

from activesetmethods_amd import acopf, problems
from tests.test_nlhess_cpu import PARITY, all_ops_model, store_model
from tests.test_nlparams_gpu import _handle_for, _same_run

pytestmark = pytest.mark.gpu
ERR_ARG, ERR_STATE = -1, -3
VALS = [(0.5, 4.0), (0.6, 4.5), (0.3, 3.0), (0.7, 6.0), (0.45, 5.5)]       # (a, p) of the parameterised model's scenarios


def _twin(fm, x, sigma, lam):
    h = fm.hessian_lagrangian_structure()
    return fm.eval_hessian_lagrangian(np.asarray(x, float), sigma, np.asarray(lam, float), np.zeros(len(h)))


def _per_handle(fms, X, sigmas, L, V):
    """Values and products of scenario s from a fresh handle set up with fms[s] (its own data), through the per-handle entries."""
    vals, prods = [], []
    for s, fm in enumerate(fms):
        opt = _handle_for(fm.to_problem(), fm)
        vals.append(opt.eval_hessian_lagrangian(X[s], float(sigmas[s]), L[s]))
        prods.append(opt.hessian_product(X[s], float(sigmas[s]), L[s], V[s]))
        opt.close()
    return np.stack(vals), np.stack(prods)


def _points(fms, seed, spread=0.05):
    rng = np.random.default_rng(seed)
    n, m, S = fms[0].n, fms[0].m, len(fms)
    X = np.stack([fm.start_point() + spread * rng.uniform(-1, 1, n) for fm in fms])
    return X, rng.standard_normal((S, m)), rng.standard_normal((S, n))


def _structure(hb):
    rows, cols = hb.hessian_structure()
    return list(zip(rows.tolist(), cols.tolist()))


def test_structure_equals_the_per_handle_one_and_the_twin():
    from activesetmethods_amd import batch
    base = acopf.synthetic_case("case118", 1, 0.5)
    for name, fm in (("hs071", problems.hs071_function_model()), ("store", store_model()), ("acopf expr", acopf.function_model(base, nlp="expr"))):
        pr = fm.to_problem(name)
        opt = _handle_for(pr, fm)
        rows, cols = opt.hessian_structure()
        opt.close()
        hb = batch.HipBatch(pr, 2)
        nnz = C.c_int64(-1)
        assert hb._lib.asm_batch_hessian_structure(hb._b, C.byref(nnz), None, None) == 0 and nnz.value == len(rows), name       # nnz-only query
        got = _structure(hb)
        assert got == list(zip(rows.tolist(), cols.tolist())) == fm.hessian_lagrangian_structure(), name
        assert hb.hessian_structure()[0].dtype == np.int64
        hb.close()
    assert (fm.n, fm.m) != (4, 2) and len(got) > 1000         # the last model is the large one


@functools.lru_cache(maxsize=None)
def _parametric_reference():
    """The five scenarios of the parameterised model: points, the per-handle device results on fresh handles for the mixed obj_factor
    array and for obj_factor 1 everywhere, and the setup-data (scenario 0's) results at the same points.  Computed once, never changed."""
    fms = [problems.parametric_function_model(a, p) for a, p in VALS]
    X, L, V = _points(fms, 5, 0.3)
    sig = np.array([1.0, 0.0, 1.0, 1.0, 0.0])
    ones = np.ones(5)
    ref = dict(fms=fms, X=X, L=L, V=V, sig=sig, mixed=_per_handle(fms, X, sig, L, V), ones=_per_handle(fms, X, ones, L, V),
               setup=_per_handle([fms[0]] * 5, X, ones, L, V))
    for k in ("mixed", "ones", "setup"):
        for a in ref[k]:
            a.setflags(write=False)
    return ref


@pytest.mark.parametrize("slots,groups", [(5, 1), (5, 2), (2, 1)])
def test_per_scenario_data_is_bit_identical_to_fresh_handles_and_the_twin(slots, groups):
    """Five scenarios with their own (a, p) in the table: as many slots as scenarios in one group and in two, and two slots (a slot must
    replace an earlier scenario's data); a per-scenario obj_factor array mixing 1.0 and 0.0, and NULL."""
    from activesetmethods_amd import batch
    ref = _parametric_reference()
    fms, X, L, V = ref["fms"], ref["X"], ref["L"], ref["V"]
    hb = batch.HipBatch(fms[0].to_problem(), slots, groups=groups)
    assert hb.groups == groups
    hb.set_scenario_data(np.asarray(VALS))
    for sig, key in ((ref["sig"], "mixed"), (None, "ones")):
        want_v, want_p = ref[key]
        if sig is None:                                       # NULL obj_factor through the C ABI
            from activesetmethods_amd import _lib
            got_v, got_p = np.empty_like(want_v), np.empty_like(want_p)
            hb._check(hb._lib.asm_batch_hessian_lagrangian(hb._b, 5, _lib.dptr(X), None, _lib.dptr(L), _lib.dptr(got_v)))
            hb._check(hb._lib.asm_batch_hessian_product(hb._b, 5, _lib.dptr(X), None, _lib.dptr(L), _lib.dptr(V), _lib.dptr(got_p)))
        else:
            got_v, got_p = hb.eval_hessian_lagrangian(X, sig, L), hb.hessian_product(X, sig, L, V)
        assert got_v.shape == want_v.shape and got_p.shape == (5, 2)
        for s, fm in enumerate(fms):
            sg = 1.0 if sig is None else float(sig[s])
            assert np.array_equal(got_v[s], want_v[s]) and np.array_equal(got_p[s], want_p[s]), (key, s)
            assert np.array_equal(got_v[s], _twin(fm, X[s], sg, L[s])), (key, s)
            assert np.array_equal(got_p[s], fm.hessian_lagrangian_product(X[s], sg, L[s], V[s])), (key, s)
    assert not np.array_equal(ref["ones"][0][0], ref["ones"][0][1])          # the scenarios' Hessians do differ
    hb.close()


def test_without_a_table_after_a_table_every_scenario_has_the_setup_data():
    from activesetmethods_amd import batch
    ref = _parametric_reference()
    fms, X, L, V = ref["fms"], ref["X"], ref["L"], ref["V"]
    hb = batch.HipBatch(fms[0].to_problem(), 2)
    hb.set_scenario_data(np.asarray(VALS))
    assert np.array_equal(hb.eval_hessian_lagrangian(X, 1.0, L), ref["ones"][0])
    hb.set_scenario_data(None)                                # count = 0
    assert np.array_equal(hb.eval_hessian_lagrangian(X, 1.0, L), ref["setup"][0])
    assert np.array_equal(hb.hessian_product(X, 1.0, L, V), ref["setup"][1])
    assert np.array_equal(hb.eval_hessian_lagrangian(X[:3], 1.0, L[:3]), ref["setup"][0][:3])       # any scenario count without a table
    hb.close()


def _parity(got, want, what):
    bar = PARITY * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(got - want).max())
    print("%s: max |device - twin| = %.3e, bar %.3e" % (what, err, bar))
    assert np.all(np.abs(got - want) <= bar), what


def test_acopf_line_scenarios_on_two_slots():
    """Five case118-sized line scenarios of the expression ACOPF with branch parameters, two slots: bit-identical to a fresh handle per
    scenario, within the parity bar of the host twin."""
    from activesetmethods_amd import batch
    base = acopf.synthetic_case("case118", 1, 0.5)
    fms = [acopf.function_model(acopf.line_scenario_case(base, s), nlp="expr", branch_params=True) for s in range(5)]
    prs = [fm.to_problem("line scenario %d" % s) for s, fm in enumerate(fms)]
    X, L, V = _points(fms, 8, 0.01)
    sig = np.array([1.0, 0.5, 0.0, 1.0, 2.0])
    want_v, want_p = _per_handle(fms, X, sig, L, V)
    hb = batch.HipBatch(prs[0], 2)
    data = hb.scenario_data(prs)
    assert data is not None and data.shape[0] == 5
    hb.set_scenario_data(data)
    got_v, got_p = hb.eval_hessian_lagrangian(X, sig, L), hb.hessian_product(X, sig, L, V)
    hb.close()
    assert np.array_equal(got_v, want_v) and np.array_equal(got_p, want_p)
    assert not np.array_equal(got_v[0], got_v[1])
    for s, fm in enumerate(fms):
        _parity(got_v[s], _twin(fm, X[s], sig[s], L[s]), "scenario %d values" % s)
        _parity(got_p[s], fm.hessian_lagrangian_product(X[s], sig[s], L[s], V[s]), "scenario %d product" % s)


def test_all_ops_tape_without_a_table():
    from activesetmethods_amd import batch
    fm = all_ops_model()
    rng = np.random.default_rng(11)
    X, L, V = rng.uniform(0.4, 1.1, (3, 4)), rng.standard_normal((3, fm.m)), rng.standard_normal((3, 4))
    sig = np.array([1.0, 0.0, 0.7])
    want_v, want_p = _per_handle([fm] * 3, X, sig, L, V)
    hb = batch.HipBatch(fm.to_problem(), 2)
    got_v, got_p = hb.eval_hessian_lagrangian(X, sig, L), hb.hessian_product(X, sig, L, V)
    hb.close()
    assert np.array_equal(got_v, want_v) and np.array_equal(got_p, want_p)
    for s in range(3):
        _parity(got_v[s], _twin(fm, X[s], sig[s], L[s]), "all ops %d values" % s)
        _parity(got_p[s], fm.hessian_lagrangian_product(X[s], sig[s], L[s], V[s]), "all ops %d product" % s)


def test_the_slots_launches_are_merged():
    """Eight slots in one group, eight scenarios: launches made per operation recorded, for one Hessian call (the first, which also
    clears the slots' new workspaces, and a later one) and for asm_batch_data_gradient on the same batch - the Hessian kernels merge no
    worse than the kernels that have been merging since before them."""
    from activesetmethods_amd import batch
    fms = [problems.parametric_function_model(0.3 + 0.05 * s, 3.0 + 0.5 * s) for s in range(8)]
    X, L, _ = _points(fms, 2, 0.3)
    hb = batch.HipBatch(fms[0].to_problem(), 8, groups=1)
    hb.set_scenario_data(np.asarray([fm.nlp.device[2] for fm in fms], float))
    hb.hessian_structure()

    def ratio(call):
        s0 = hb.stats()
        call()
        s1 = hb.stats()
        ops, launches = s1["ops"] - s0["ops"], s1["launches"] - s0["launches"]
        assert ops > 0 and launches > 0
        return launches / ops, ops, launches

    first = ratio(lambda: hb.eval_hessian_lagrangian(X, 1.0, L))
    later = ratio(lambda: hb.eval_hessian_lagrangian(X, 1.0, L))
    grad = ratio(lambda: hb.data_gradient(X, L))
    hb.close()
    print("launches / operations: first Hessian call %.4f (%d ops, %d launches), later call %.4f (%d, %d), data gradient %.4f (%d, %d)"
          % (first + later + grad))
    assert first[0] <= grad[0] and later[0] <= grad[0]
    assert later[2] < later[1] / 4                            # eight slots: far fewer launches than operations


def test_hessian_calls_do_not_interfere_with_the_batch():
    """A 3-LP asm_batch_slp_run on hs071 scenarios gives the same bits with Hessian calls before and between the runs as without; after a
    second set-up with another model the structure call gives the new model's pattern."""
    import activesetmethods_amd as A
    from activesetmethods_amd import batch
    fm = problems.hs071_function_model()
    pr = fm.to_problem()
    par = A.Parameters(algorithm="Line Search", max_iter=60, device_eval=True)
    rng = np.random.default_rng(3)
    S = 3
    st = lambda k: np.stack([getattr(pr, k)] * S)
    x0 = np.clip(st("x0") + 0.05 * rng.uniform(-1, 1, (S, pr.n)), pr.x_L, pr.x_U)
    lam, v = rng.standard_normal((S, pr.m)), rng.standard_normal((S, pr.n))
    outs = []
    for hess in (False, True):
        hb = batch.HipBatch(pr, 2)
        if hess:
            hb.eval_hessian_lagrangian(0.5 * x0 + 0.1, 1.0, lam)
            hb.hessian_structure()
        r1 = hb.slp_run(st("g_L"), st("g_U"), st("x_L"), st("x_U"), x0, par, max_lp_solves=3)
        if hess:
            hb.hessian_product(np.stack([r.x for r in r1]), 0.5, -np.stack([r.lam for r in r1]), v)
            hb.eval_hessian_lagrangian(x0, [1.0, 0.0, 1.0], lam)
        r2 = hb.slp_run(st("g_L"), st("g_U"), st("x_L"), st("x_U"), x0, par, max_lp_solves=3)
        outs.append((r1, r2))
        if hess:
            assert _structure(hb) == fm.hessian_lagrangian_structure()
            te = problems.toy_expr_function_model()
            hb.setup(te.to_problem())
            assert _structure(hb) == te.hessian_lagrangian_structure() != fm.hessian_lagrangian_structure()
            xt, lt = np.array([[-1.3, 0.8], [0.4, 0.9]]), rng.standard_normal((2, te.m))
            got = hb.eval_hessian_lagrangian(xt, 1.0, lt)
            assert all(np.array_equal(got[s], _twin(te, xt[s], 1.0, lt[s])) for s in range(2))
        hb.close()
    (a1, a2), (b1, b2) = outs
    assert all(1 <= r.lp_solves <= 3 for r in a1)
    for ra, rb in zip(a1 + a2, b1 + b2):
        _same_run(ra, rb)


def test_argument_and_state_errors():
    import activesetmethods_amd as A
    from activesetmethods_amd import _lib, batch
    lib = _lib.load()
    ref = _parametric_reference()
    fm, X, L, V = ref["fms"][0], ref["X"], ref["L"], ref["V"]
    pr = fm.to_problem()
    d, i64 = _lib.dptr, _lib.i64ptr
    nnz = C.c_int64(0)
    rows, cols, vals, out = np.zeros(8, np.int64), np.zeros(8, np.int64), np.zeros((5, 8)), np.zeros((5, 2))

    def calls(b):
        return (lib.asm_batch_hessian_structure(b, C.byref(nnz), None, None), lib.asm_batch_hessian_lagrangian(b, 5, d(X), None, d(L), d(vals)),
                lib.asm_batch_hessian_product(b, 5, d(X), None, d(L), d(V), d(out)))

    raw = C.c_void_p()
    assert lib.asm_batch_create(0, 2, C.byref(raw)) == 0
    assert calls(raw) == (ERR_STATE,) * 3                                                              # before asm_batch_setup
    jr, jc = np.ascontiguousarray(pr.j_row, np.int64), np.ascontiguousarray(pr.j_col, np.int64)
    assert lib.asm_batch_setup(raw, pr.n, pr.m, len(jr), i64(jr), i64(jc), d(pr.g_L), d(pr.g_U), d(pr.x_L), d(pr.x_U)) == 0
    assert calls(raw) == (ERR_STATE,) * 3                                                              # before asm_batch_eval_setup
    assert lib.asm_batch_destroy(raw) == 0
    assert calls(None) == (ERR_ARG,) * 3                                                               # null batch

    hb = batch.HipBatch(pr, 2)
    b = hb._b
    want = ref["setup"][0]

    def still_works():
        assert np.array_equal(hb.eval_hessian_lagrangian(X, 1.0, L), want)

    still_works()
    assert lib.asm_batch_hessian_structure(b, None, None, None) == ERR_ARG
    assert lib.asm_batch_hessian_structure(b, C.byref(nnz), i64(rows), None) == ERR_ARG                # rows without cols
    assert lib.asm_batch_hessian_structure(b, C.byref(nnz), None, i64(cols)) == ERR_ARG
    still_works()
    for bad in range(3):
        a = [d(X), d(L), d(vals)]
        a[bad] = None
        assert lib.asm_batch_hessian_lagrangian(b, 5, a[0], None, a[1], a[2]) == ERR_ARG, bad
        still_works()
    for bad in range(4):
        a = [d(X), d(L), d(V), d(out)]
        a[bad] = None
        assert lib.asm_batch_hessian_product(b, 5, a[0], None, a[1], a[2], a[3]) == ERR_ARG, bad
    still_works()
    for n_scen in (0, -1):
        assert lib.asm_batch_hessian_lagrangian(b, n_scen, d(X), None, d(L), d(vals)) == ERR_ARG
        assert lib.asm_batch_hessian_product(b, n_scen, d(X), None, d(L), d(V), d(out)) == ERR_ARG
    still_works()
    hb.set_scenario_data(np.asarray(VALS[:3]))                                                         # a table of 3 scenarios against 5
    assert lib.asm_batch_hessian_lagrangian(b, 5, d(X), None, d(L), d(vals)) == ERR_ARG
    assert lib.asm_batch_hessian_product(b, 5, d(X), None, d(L), d(V), d(out)) == ERR_ARG
    with pytest.raises(A.AsmHipError, match="scenario"):
        hb.eval_hessian_lagrangian(X, 1.0, L)
    assert np.array_equal(hb.eval_hessian_lagrangian(X[:3], 1.0, L[:3]), ref["ones"][0][:3])           # 3 against 3: the table's data
    hb.set_scenario_data(None)
    still_works()
    with pytest.raises(ValueError):
        hb.eval_hessian_lagrangian(X[:, :1], 1.0, L)                                                   # shapes: refused in Python
    with pytest.raises(ValueError):
        hb.hessian_product(X, np.ones(4), L, V)
    hb.close()

    for fk in (acopf.function_model(acopf.synthetic_case("case118", 1, 0.5)), problems.synthetic_dense_function_model(40, 10)):      # kinds 1 and 2
        pk = fk.to_problem()
        hk = batch.HipBatch(pk, 2)
        xk, lk = np.stack([pk.x0] * 2), np.zeros((2, pk.m))
        assert lib.asm_batch_hessian_structure(hk._b, C.byref(nnz), None, None) == ERR_ARG
        assert lib.asm_batch_hessian_lagrangian(hk._b, 2, d(xk), None, d(lk), d(np.zeros((2, 8)))) == ERR_ARG
        assert lib.asm_batch_hessian_product(hk._b, 2, d(xk), None, d(lk), d(xk), d(np.zeros_like(xk))) == ERR_ARG
        with pytest.raises(A.AsmHipError, match="second derivatives"):
            hk.hessian_structure()
        f, df, E = C.c_double(0.0), np.zeros(pk.n), np.zeros(pk.m)                                     # the batch still evaluates functions
        h0 = C.c_void_p(lib.asm_batch_handle(hk._b, 0))
        assert lib.asm_eval_functions(h0, d(np.ascontiguousarray(pk.x0, np.float64)), C.byref(f), d(df), d(E)) == 0
        assert np.isfinite(f.value) and np.all(np.isfinite(E)) and np.all(np.isfinite(df))
        hk.close()


@pytest.mark.parametrize("sparse", [False, True])
def test_lagrangian_hessians_equal_the_twin_at_the_batch_solutions(sparse):
    """The converged runs of the parameterised scenarios (three of them, two slots): batch.lagrangian_hessians equals
    moi_evaluator.lagrangian_hessian of each scenario's model at the run's (x, lam), bit for bit, dense and scipy.sparse."""
    import activesetmethods_amd as A
    from activesetmethods_amd import batch
    from activesetmethods_amd.moi_evaluator import lagrangian_hessian
    fms = [problems.parametric_function_model(a, p) for a, p in VALS[:3]]
    prs = [fm.to_problem("parametric %d" % s) for s, fm in enumerate(fms)]
    st = lambda k: np.stack([getattr(p, k) for p in prs])
    hb = batch.HipBatch(prs[0], 2)
    par = A.Parameters(algorithm="Trust Region", max_iter=60, device_eval=True)
    runs = hb.slp_run(st("g_L"), st("g_U"), st("x_L"), st("x_U"), st("x0"), par, data=hb.scenario_data(prs))
    assert all(r.ret == 0 for r in runs)
    Hs = batch.lagrangian_hessians(hb, runs, sparse=sparse)
    hb.close()
    assert len(Hs) == 3
    for s, (fm, r) in enumerate(zip(fms, runs)):
        want = lagrangian_hessian(fm, r.x, r.lam, sparse=sparse)
        if sparse:
            assert Hs[s].shape == want.shape == (2, 2) and Hs[s].format == "csr"
            assert np.array_equal(Hs[s].toarray(), want.toarray())
        else:
            assert np.array_equal(Hs[s], want) and np.array_equal(Hs[s], Hs[s].T)
    assert not np.array_equal(np.asarray(Hs[0].todense() if sparse else Hs[0]), np.asarray(Hs[1].todense() if sparse else Hs[1]))
