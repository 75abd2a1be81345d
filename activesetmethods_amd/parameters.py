"""`Parameters` with the reference's names and defaults (src/parameters.jl:1-29).  `external_optimizer`
keeps its role as the plugin slot (src/parameters.jl:7, consumed at src/algorithms/slp.jl:32): here it
is a factory `(data, j_row, j_col) -> AbstractSubOptimizer`; unset selects the HIP sub-optimizer."""
from dataclasses import dataclass
from typing import Any


@dataclass
class Parameters:
    mode: str = "Normal"
    method: str = "SLP"
    algorithm: str = "Line Search"
    external_optimizer: Any = None
    hessian_type: str = "none"
    OutputFlag: int = 0
    StatisticsFlag: int = 0
    tol_direction: float = 1.e-6
    tol_residual: float = 0.01
    tol_infeas: float = 0.01
    max_iter: int = 1000
    time_limit: float = float("inf")
    mu_merit: float = float("inf")
    max_mu: float = 1.e+6
    rho: float = 0.8
    eta: float = 0.4
    tau: float = 0.9
    min_alpha: float = 1.e-6
    tr_size: float = 0.4
    # not in the reference: evaluate f, grad f, g and the Jacobian values on the GPU (needs a Problem built from a FunctionModel,
    # activesetmethods_amd/moi_evaluator.py) and run the per-iteration norms / merit reductions there
    device_eval: bool = False
    # not in the reference: algorithm = "SLP-EQP" (slp.SlpEQP, asm_slp_run_eqp) - the initial radius of its trust-region step (None:
    # tr_size), the cap on that radius, the activity tolerance of its working set, and a switch that leaves the Trust Region driver
    eqp_radius: Any = None
    eqp_radius_max: float = 1.e+3
    eqp_tol_active: float = 1.e-8
    eqp: bool = True
    # not in the reference: the form of the KKT solves behind the SLP-EQP step (asm_kkt_set_form) - "dense" or "sparse" (sparse products, a
    # banded factor of A A' in a reverse Cuthill-McKee order of the working rows).  kkt_order (asm_kkt_set_order), the row order of the
    # sparse form: "working-set" orders every new working set on the host, "static" restricts one order of all rows, made once.  The
    # scenario batches run "sparse" in the "static" order only.
    kkt_form: str = "dense"
    kkt_order: str = "working-set"
    # `hessian_type` (above, src/parameters.jl:9-10: "approximation hessian (limited-memory), exact, or none") is read by SLP-EQP: "none" and
    # "exact" use the model's own second derivatives, "limited-memory" a limited-memory BFGS approximation of the Hessian of the Lagrangian
    # held on the device (asm_hessian_set_type) - for models without second derivatives.  lm_memory: the pairs it keeps (1 .. 32).  Per
    # handle only: the scenario batches refuse "limited-memory".  The derivative entries (Hessians, data gradients, cross derivatives,
    # sensitivities) stay exact whatever the type: they need an expression block or a block kernel with its derivative entries
    # (acopf.function_model(case, hessian=True), problems.synthetic_dense_function_model(n, m, hessian=True): device kinds 4 and 5).
    lm_memory: int = 10

    def __post_init__(self):
        check_kkt_form(self.kkt_form)
        check_kkt_order(self.kkt_order)
        check_hessian_type(self.hessian_type)
        if not 1 <= int(self.lm_memory) <= 32:
            raise ValueError("lm_memory = %r: expected 1 .. 32" % (self.lm_memory,))


KKT_FORMS = ("dense", "sparse")
KKT_ORDERS = ("working-set", "static")
HESSIAN_TYPES = ("none", "exact", "limited-memory")


def check_hessian_type(kind):
    if kind not in HESSIAN_TYPES:
        raise ValueError("hessian_type = %r: expected \"none\", \"exact\" or \"limited-memory\"" % (kind,))
    return kind


def check_kkt_form(form):
    if form not in KKT_FORMS:
        raise ValueError("kkt_form = %r: expected \"dense\" or \"sparse\"" % (form,))
    return form


def check_kkt_order(order):
    if not isinstance(order, str) or order not in KKT_ORDERS:
        raise ValueError("kkt_order = %r: expected \"working-set\" or \"static\"" % (order,))
    return order


def get_parameter(params, pname):          # src/parameters.jl:31-33
    return getattr(params, pname)


def set_parameter(params, pname, val):     # src/parameters.jl:35-38
    if not hasattr(params, pname):
        raise AttributeError(pname)
    setattr(params, pname, val)
