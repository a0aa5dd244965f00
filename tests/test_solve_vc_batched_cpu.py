"""The batched variable-coefficient solver (include/mg_varcoef_batch.h) without a GPU: the header against the binding and the
library's exports, its place in mg_hip.h, mg_varcoef.h's unchanged surface, the docstrings, and the constructors that keep
refusing a `coef` argument."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mg_batch_solver_set_coefficient", "mg_batch_solver_has_coefficient")
VC_SYMBOLS = ("mg_solver_set_coefficient", "mg_solver_has_coefficient", "mg_applyOperator", "mg_coarsenCoefficient",
              "mg_sweepCoefficient", "mg_residualCoefficient")


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text, names = declared("mg_varcoef_batch.h")
    assert names == sorted(SYMBOLS)
    assert sorted(m.ABI_VC_BATCH) == names
    lib = m.load_library()
    for name in names:
        assert name not in m.ABI and name not in m.ABI_VC and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == m.ABI_VC_BATCH[name][1]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_VC_BATCH[name][1]), name
    assert b"0.2.2" in lib.mg_version()


def test_mg_hip_includes_the_header_after_mg_heat_vc():
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    order = [hip.index('#include "%s"' % h) for h in ("mg_varcoef.h", "mg_heat_vc.h", "mg_varcoef_batch.h")]
    assert order == sorted(order)
    # (the batch solver's type is declared before the header that uses it)
    assert hip.index("typedef struct mg_batch_solver mg_batch_solver;") < order[-1]


def test_mg_varcoef_h_declares_what_it_declared():
    import multigrid_poisson_solver_amd as m
    assert declared("mg_varcoef.h")[1] == sorted(VC_SYMBOLS) == sorted(m.ABI_VC)


def test_docstrings_state_the_contract():
    import multigrid_poisson_solver_amd as m
    for f in (m.BatchSolver, m.BatchSolver.set_coefficient, m.solve_batched_coef):
        doc = " ".join(f.__doc__.split())
        assert "bit" in doc and ("Solver(coef=a" in doc or "coef=a_i" in doc), f.__qualname__
    doc = " ".join(m.BatchSolver.set_coefficient.__doc__.split())
    for phrase in ("(N, N)", "(n, N, N)", "shared", "None", "a == 1", "max_batch", "leaves the solver as it was"):
        assert phrase in doc, phrase
    assert isinstance(m.BatchSolver.has_coefficient, property) and isinstance(m.BatchSolver.n_coefficients, property)
    assert m.BatchSolver.has_coefficient.__doc__ and m.BatchSolver.n_coefficients.__doc__


def test_signatures_that_take_no_coefficient_are_unchanged():
    import multigrid_poisson_solver_amd as m
    assert list(inspect.signature(m.BatchSolver.__init__).parameters) == ["self", "N", "L", "max_batch", "opts"]
    assert list(inspect.signature(m.solve_batched).parameters) == ["F", "U", "L", "opts"]
    assert "coef" not in inspect.signature(m.HeatStepper.__init__).parameters
    assert list(inspect.signature(m.solve_batched_coef).parameters) == ["F", "a", "U", "L", "opts"]
    assert list(inspect.signature(m.BatchSolver.set_coefficient).parameters) == ["self", "a"]
    assert "coef" not in {f for f, _ in m.SolveOpts._fields_}
