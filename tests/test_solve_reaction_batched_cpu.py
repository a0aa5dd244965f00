"""The batched solver with a reaction term (include/mg_rx_batch.h) without a GPU: the header against the binding and the
library's exports, its one include line in mg_hip.h, the build's sources, the Python signatures -- the new ones and the ones
that must not change -- and the docstrings."""
import inspect
import os
import re


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mg_batch_solver_set_reaction", "mg_batch_solver_has_reaction")


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text, names = declared("mg_rx_batch.h")
    assert names == sorted(SYMBOLS)
    assert sorted(m.ABI_RX_BATCH) == names
    lib = m.load_library()
    for name in names:
        for other in (m.ABI, m.ABI_VC_BATCH, m.ABI_REACTION, m.ABI_KRYLOV_BATCH):
            assert name not in other, name
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == m.ABI_RX_BATCH[name][1] and getattr(lib, name).restype is m.ABI_RX_BATCH[name][0]
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(m.ABI_RX_BATCH[name][1]), name
    # the setter mirrors mg_batch_solver_set_coefficient
    assert m.ABI_RX_BATCH["mg_batch_solver_set_reaction"] == m.ABI_VC_BATCH["mg_batch_solver_set_coefficient"]
    assert m.ABI_RX_BATCH["mg_batch_solver_has_reaction"] == m.ABI_VC_BATCH["mg_batch_solver_has_coefficient"]


def test_mg_hip_includes_the_header_on_one_line_after_mg_newton():
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert hip.count('#include "mg_rx_batch.h"') == 1
    lines = [l.strip() for l in hip.splitlines()]
    at = lines.index('#include "mg_rx_batch.h"')
    assert lines[at - 1] == '#include "mg_newton.h"'
    assert hip.index('#include "mg_rx_batch.h"') < hip.index('#include "mg_bc.h"')
    # (the batch solver's type is declared before the header that uses it)
    assert hip.index("typedef struct mg_batch_solver mg_batch_solver;") < hip.index('#include "mg_rx_batch.h"')
    # mg_hip.h itself still speaks of the reaction in the single solver's include line alone, and its end is what it was
    assert "reaction" not in hip.replace('#include "mg_reaction.h"', "").lower()
    includes = re.findall(r'#include "([^"]+)"', hip)
    assert includes[-3:] == ["mg_bc.h", "mg_krylov_batch.h", "mg_krylov.h"]


def test_build_names_the_new_files():
    src = open(os.path.join(ROOT, "multigrid_poisson_solver_amd", "build.py")).read()
    assert '"mg_reaction_batch_kernels.hip"' in src and '"mg_rx_batch.h"' in src and "mg_reaction_impl.h" in src
    from multigrid_poisson_solver_amd import build
    assert "mg_reaction_batch_kernels.hip" in build.SOURCES
    assert os.path.join(ROOT, "include", "mg_rx_batch.h") in build._deps()
    assert os.path.exists(os.path.join(build.CSRC, "mg_reaction_batch_kernels.hip"))


def test_signatures():
    import multigrid_poisson_solver_amd as m
    assert list(inspect.signature(m.BatchSolver.set_reaction).parameters) == ["self", "s"]
    assert isinstance(m.BatchSolver.has_reaction, property) and isinstance(m.BatchSolver.n_reactions, property)
    sig = inspect.signature(m.solve_batched_reaction)
    assert list(sig.parameters) == ["F", "s", "U", "L", "coef", "krylov", "opts"]
    assert [sig.parameters[p].default for p in ("U", "L", "coef", "krylov")] == [None, 1.0, None, 0]
    # the ones that stay
    assert list(inspect.signature(m.BatchSolver.__init__).parameters) == ["self", "N", "L", "max_batch", "opts"]
    assert list(inspect.signature(m.BatchSolver.set_coefficient).parameters) == ["self", "a"]
    assert list(inspect.signature(m.BatchSolver.set_krylov).parameters) == ["self", "m"]
    assert list(inspect.signature(m.solve_batched).parameters) == ["F", "U", "L", "opts"]
    assert list(inspect.signature(m.solve_batched_coef).parameters) == ["F", "a", "U", "L", "opts"]
    assert list(inspect.signature(m.solve_batched_krylov).parameters) == ["F", "m", "U", "L", "coef", "opts"]
    assert list(inspect.signature(m.Solver.set_reaction).parameters) == ["self", "s"]
    # BatchSolver takes no reaction=, and it is no solve option either (tests/test_solve_reaction_gpu.py: a TypeError)
    assert "reaction" not in {f for f, _ in m.SolveOpts._fields_}


def test_docstrings_state_the_contract():
    import multigrid_poisson_solver_amd as m
    for f in (m.BatchSolver, m.BatchSolver.set_reaction, m.solve_batched_reaction):
        doc = " ".join(f.__doc__.split())
        assert "bit" in doc and "reaction=s" in doc and "coef=a_i" in doc, f.__qualname__
    doc = " ".join(m.BatchSolver.set_reaction.__doc__.split())
    for phrase in ("(N, N)", "(n, N, N)", "shared", "None", "s == 0", "s == c", "max_batch", ">= 0", "any order",
                   "leaves the solver as it was", "adjoint"):
        assert phrase in doc, phrase
    assert m.BatchSolver.has_reaction.__doc__ and m.BatchSolver.n_reactions.__doc__
    header = " ".join(open(os.path.join(ROOT, "include", "mg_rx_batch.h")).read().replace("\n *", "\n").split())
    for phrase in ("bit for bit", "mg_solver_set_reaction(s_i)", "instance <i>", "(nl - 1)*(pre + post + 3) + 1", "MG_ERR_UNSUPPORTED",
                   "Not built"):
        assert phrase in header, phrase
    single = open(os.path.join(ROOT, "include", "mg_reaction.h")).read()
    assert "mg_rx_batch.h" in single and "heat stepper and the eigensolver have no reaction" in single
