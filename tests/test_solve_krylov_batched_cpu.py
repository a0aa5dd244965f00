"""The batched Krylov acceleration (include/mg_krylov_batch.h) without a GPU: the header against the binding and the library's
exports, its place in mg_hip.h, signatures and docstrings, and -- on the numpy restatement of the method
(tests/_krylov_ref.py) -- the input of the batched GPU test on which two instances of one batch sit at DIFFERENT k in the same
iteration: one restarted on its recurred norm, found the recomputed norm above its tolerance and went on from k = 0 while its
neighbour carried on."""
import inspect
import os
import re

import pytest

import _krylov_ref as kref
import _solve_ref as ref
import _solve_vc_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mg_batch_solver_set_krylov", "mg_batch_solver_krylov", "mg_batch_solver_krylov_breakdown", "mg_batch_solver_krylov_log")
KRYLOV_SYMBOLS = ("mg_solver_set_krylov", "mg_solver_krylov", "mg_solver_krylov_breakdown", "mg_solver_krylov_log", "mg_krylovDots",
                  "mg_krylovOrth", "mg_krylovUpdate")

# the inputs on which the k of two instances diverge: (N, field, m, rtol, max_cycles, the two seeds of F, U0)
DIVERGING = [(33, "smooth", 4, 1e-14, 30, (1, 2)), (65, "jump", 8, 1e-13, 30, (2, 3))]


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text, names = declared("mg_krylov_batch.h")
    assert names == sorted(SYMBOLS) == sorted(m.ABI_KRYLOV_BATCH)
    lib = m.load_library()
    others = (m.ABI, m.ABI_FMG, m.ABI_HEAT, m.ABI_VC, m.ABI_HEAT_VC, m.ABI_VC_BATCH, m.ABI_KRYLOV)
    for name in names:
        assert not any(name in abi for abi in others), name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == m.ABI_KRYLOV_BATCH[name][1]
        assert getattr(lib, name).restype is m.ABI_KRYLOV_BATCH[name][0]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_KRYLOV_BATCH[name][1]), name
    assert b"0.2.2" in lib.mg_version()
    # mg_krylov.h keeps its seven names
    assert declared("mg_krylov.h")[1] == sorted(KRYLOV_SYMBOLS) == sorted(m.ABI_KRYLOV)


def test_mg_hip_includes_the_header_after_the_batch_solver_and_before_mg_krylov():
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    includes = re.findall(r'#include "(mg_\w+\.h)"', hip)
    assert includes[-2:] == ["mg_krylov_batch.h", "mg_krylov.h"]
    assert hip.index("typedef struct mg_batch_solver mg_batch_solver;") < hip.index('#include "mg_krylov_batch.h"')
    # the header is the batched form's specification and refers to mg_krylov.h for the method
    text = open(os.path.join(ROOT, "include", "mg_krylov_batch.h")).read()
    assert "mg_krylov.h" in text and "independent of the number of instances" in " ".join(text.split())


def test_signatures():
    import multigrid_poisson_solver_amd as m
    assert list(inspect.signature(m.BatchSolver.__init__).parameters) == ["self", "N", "L", "max_batch", "opts"]
    assert list(inspect.signature(m.BatchSolver.set_krylov).parameters) == ["self", "m"]
    assert list(inspect.signature(m.BatchSolver.krylov_log).parameters) == ["self", "i"]
    assert isinstance(m.BatchSolver.krylov, property) and m.BatchSolver.krylov.__doc__
    assert list(inspect.signature(m.solve_batched_krylov).parameters) == ["F", "m", "U", "L", "coef", "opts"]
    assert list(inspect.signature(m.solve_batched).parameters) == ["F", "U", "L", "opts"]
    assert list(inspect.signature(m.solve_batched_coef).parameters) == ["F", "a", "U", "L", "opts"]
    assert "krylov" not in {f for f, _ in m.SolveOpts._fields_}


def test_docstrings_state_the_contract_the_memory_and_the_recomputed_residual():
    import multigrid_poisson_solver_amd as m
    for f in (m.BatchSolver.set_krylov, m.solve_batched_krylov):
        doc = " ".join(f.__doc__.split())
        assert "GCR(m)" in doc and "bit-identical" in doc and "krylov=m" in doc, f.__qualname__
        assert "(2m + 1)*N^2" in doc and "recomputed residual" in doc, f.__qualname__
    doc = " ".join(m.BatchSolver.set_krylov.__doc__.split())
    for phrase in ("max_batch", "a solve allocates nothing", "leaves the solver as it was", "set_coefficient", "m = 0"):
        assert phrase in doc, phrase
    assert "set_krylov" in " ".join(m.BatchSolver.__doc__.split())
    assert "Solver.krylov_log" in " ".join(m.BatchSolver.krylov_log.__doc__.split())


@pytest.mark.parametrize("N,name,m,rtol,max_cycles,seeds", DIVERGING)
def test_two_instances_sit_at_different_k_in_one_iteration(oracle, N, name, m, rtol, max_cycles, seeds):
    """Measured on this restatement: N = 33 `smooth` m = 4 -- at iteration 13 seed 1 has k = 0 and seed 2 has k = 1;
    N = 65 `jump` m = 8 -- seeds 2 and 3 differ at iteration 18.  The property is asserted, not the index."""
    a = vref.field(name, N, seed=1)
    outs = []
    for seed in seeds:
        F, U0 = ref.random_problem(N, seed)
        out = kref.solve(oracle, a, F, U0, 1.0, m=m, rtol=rtol, max_cycles=max_cycles)
        assert not out["converged"] and not out["breakdown"] and out["cycles"] == max_cycles, seed
        # a restart on the recurred norm (k < m at that point) whose recomputed norm was above the tolerance
        early = [i for i, rec in enumerate(out["records"]) if rec["restarted"] and rec["k"] + 1 < m]
        assert early, seed
        for i in early:
            assert out["history"][i + 1] > out["tol"], (seed, i)
        outs.append(out)
    ks = [[rec["k"] for rec in out["records"]] for out in outs]
    differ = [i for i, (x, y) in enumerate(zip(*ks)) if x != y]
    print(f"N={N} {name} m={m}: seeds {seeds} sit at different k in iterations {differ}")
    assert differ
