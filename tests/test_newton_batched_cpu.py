"""The batched semilinear solve (include/mg_newton_batch.h) without a GPU: the header against the binding and the library's
exports (argument counts, struct fields), its one include line in mg_hip.h, the build's sources, the Python signatures and
defaults against Solver.newton's, and the tables and headers that must not change."""
import ctypes as C
import inspect
import os
import re


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mg_batch_solver_newton", "mg_batch_solver_newton_history", "mg_batch_solver_newton_inner_history",
           "mg_nonlinearResidual_batch")
NEWTON_SYMBOLS = ("mg_newton_opts_default", "mg_solver_newton", "mg_solver_newton_history", "mg_solver_newton_inner_history",
                  "mg_nonlinearResidual")
RX_BATCH_SYMBOLS = ("mg_batch_solver_set_reaction", "mg_batch_solver_has_reaction")
CTYPE = {"int": C.c_int, "double": C.c_double}


def declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return text, sorted(set(re.findall(r"\b(mg_[A-Za-z0-9_]+)\s*\(", text)))


def struct_fields(text, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            typ, names = decl.split(None, 1)
            out += [(n.strip(), CTYPE[typ]) for n in names.split(",")]
    return out


def test_header_declares_what_the_binding_binds_and_the_library_exports():
    import multigrid_poisson_solver_amd as m
    text, names = declared("mg_newton_batch.h")
    assert names == sorted(SYMBOLS)
    assert sorted(m.ABI_NEWTON_BATCH) == names
    lib = m.load_library()
    for name in names:
        for other in (m.ABI, m.ABI_NEWTON, m.ABI_RX_BATCH, m.ABI_VC_BATCH, m.ABI_KRYLOV_BATCH, m.ABI_REACTION):
            assert name not in other, name
        assert hasattr(lib, name), name
        res, args = m.ABI_NEWTON_BATCH[name]
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype is res
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1).split(",") if a.strip()])
        assert n_args == len(args), name
    assert struct_fields(text, "mg_batch_newton_stats") == list(m.BatchNewtonStats._fields_)
    # the options, the results and the records are mg_newton.h's: this header declares no struct of its own for them
    assert re.findall(r"typedef struct (\w+)", text) == ["mg_batch_newton_stats"]
    driver = m.ABI_NEWTON_BATCH["mg_batch_solver_newton"][1]
    assert driver[-3:] == [C.POINTER(m.NewtonOpts), C.POINTER(m.NewtonResult), C.POINTER(m.BatchNewtonStats)]
    assert m.ABI_NEWTON_BATCH["mg_batch_solver_newton_history"][1][2] == C.POINTER(m.NewtonIter)


def test_mg_hip_includes_the_header_on_one_line_after_mg_rx_batch():
    hip = open(os.path.join(ROOT, "include", "mg_hip.h")).read()
    assert hip.count('#include "mg_newton_batch.h"') == 1
    lines = [l.strip() for l in hip.splitlines()]
    at = lines.index('#include "mg_newton_batch.h"')
    assert lines[at - 1] == '#include "mg_rx_batch.h"' and lines[at - 2] == '#include "mg_newton.h"'
    includes = re.findall(r'#include "([^"]+)"', hip)
    assert includes[-3:] == ["mg_bc.h", "mg_krylov_batch.h", "mg_krylov.h"]
    assert "reaction" not in hip.replace('#include "mg_reaction.h"', "").lower()
    # (the types the header uses are declared before it)
    assert hip.index("typedef struct mg_batch_solver mg_batch_solver;") < hip.index('#include "mg_newton_batch.h"')
    assert hip.index('#include "mg_newton.h"') < hip.index('#include "mg_newton_batch.h"')


def test_build_names_the_new_files():
    src = open(os.path.join(ROOT, "multigrid_poisson_solver_amd", "build.py")).read()
    assert '"mg_newton_batch_kernels.hip"' in src and '"mg_newton_batch.h"' in src and "mg_newton_impl.h" in src
    from multigrid_poisson_solver_amd import build
    assert "mg_newton_batch_kernels.hip" in build.SOURCES
    assert os.path.join(ROOT, "include", "mg_newton_batch.h") in build._deps()
    assert os.path.exists(os.path.join(build.CSRC, "mg_newton_batch_kernels.hip"))
    # the batched kernels are compiled from the single kernels' bodies, not from a copy of them
    kernels = open(os.path.join(build.CSRC, "mg_newton_batch_kernels.hip")).read()
    assert '#include "mg_newton_impl.h"' in kernels and "nw_body<" in kernels and "blockIdx.z" in kernels


def test_signatures_and_defaults_equal_solver_newton():
    import multigrid_poisson_solver_amd as m
    single = inspect.signature(m.Solver.newton)
    batch = inspect.signature(m.BatchSolver.newton_batch)
    assert list(batch.parameters) == list(single.parameters) == \
        ["self", "F", "U", "kind", "kappa", "weight", "rtol", "atol", "max_iters", "max_backtracks"]
    for p in single.parameters:
        assert batch.parameters[p].default == single.parameters[p].default, p
    ptr, ptrs = inspect.signature(m.Solver.newton_ptr), inspect.signature(m.BatchSolver.newton_ptrs)
    assert list(ptrs.parameters) == ["self", "F_ptrs", "U_ptrs", "kind", "kappa", "w_ptrs", "rtol", "atol", "max_iters", "max_backtracks"]
    for a, b in zip(list(ptr.parameters)[3:], list(ptrs.parameters)[3:]):
        assert ptr.parameters[a].default == ptrs.parameters[b].default, (a, b)
    one, many = inspect.signature(m.solve_semilinear), inspect.signature(m.solve_semilinear_batched)
    assert list(many.parameters) == list(one.parameters)
    for p in one.parameters:
        assert many.parameters[p].default == one.parameters[p].default, p
    assert list(inspect.signature(m.nonlinear_residual_batch).parameters) == list(inspect.signature(m.nonlinear_residual).parameters)
    o = m.NewtonOpts()
    m.load_library().mg_newton_opts_default(C.byref(o))
    assert [batch.parameters[p].default for p in ("rtol", "atol", "max_iters", "max_backtracks")] == \
        [o.rtol, o.atol, o.max_iters, o.max_backtracks]
    # the ones that stay
    assert list(inspect.signature(m.BatchSolver.__init__).parameters) == ["self", "N", "L", "max_batch", "opts"]
    assert list(inspect.signature(m.BatchSolver.solve).parameters) == ["self", "F", "U"]
    assert list(inspect.signature(m.BatchSolver.solve_ptrs).parameters) == ["self", "F_ptrs", "U_ptrs"]
    assert not hasattr(m.HeatStepper, "newton") and not hasattr(m.EigenSolver, "newton")
    # (tests/test_newton_gpu.py pins that BatchSolver has no attribute `newton`: the batched call is newton_batch)
    assert not hasattr(m.BatchSolver, "newton")


def test_other_tables_and_mg_newton_h_are_unchanged():
    import multigrid_poisson_solver_amd as m
    assert sorted(m.ABI_NEWTON) == sorted(NEWTON_SYMBOLS) == declared("mg_newton.h")[1]
    assert sorted(m.ABI_RX_BATCH) == sorted(RX_BATCH_SYMBOLS) == declared("mg_rx_batch.h")[1]
    assert len(m.ABI_NEWTON["mg_solver_newton"][1]) == 8 and len(m.ABI_NEWTON["mg_nonlinearResidual"][1]) == 15
    assert m.ABI_RX_BATCH["mg_batch_solver_set_reaction"] == m.ABI_VC_BATCH["mg_batch_solver_set_coefficient"]
    # neither header lists the batched Newton solve as missing any more, and both point at the new one
    for header in ("mg_newton.h", "mg_rx_batch.h"):
        text = " ".join(open(os.path.join(ROOT, "include", header)).read().replace("\n *", "\n").split())
        missing = text[text.index("Not built"):]
        assert "batched Newton" not in missing and "the batched solver" not in missing, header
        assert "mg_newton_batch.h" in text, header


def test_docstrings_and_header_state_the_contract():
    import multigrid_poisson_solver_amd as m
    for f in (m.BatchSolver.newton_batch, m.solve_semilinear_batched, m.nonlinear_residual_batch):
        doc = " ".join(f.__doc__.split())
        assert "bit" in doc and "mg_newton_batch.h" in doc, f.__qualname__
    doc = " ".join(m.BatchSolver.newton_batch.__doc__.split())
    for phrase in ("lockstep", "infos.stats", "trial_rounds", "leaves the batch", "[3]", "[2]", "names the instance", "no reaction afterwards",
                   "allocate nothing"):
        assert phrase in doc, phrase
    header = " ".join(open(os.path.join(ROOT, "include", "mg_newton_batch.h")).read().replace("\n *", "\n").split())
    for phrase in ("bit for bit", "mg_solver_newton", "instance <i>", "r' < (1 - 1e-4*t)*r", "t = 2^-k", "MG_ERR_UNSUPPORTED",
                   "mg_batch_solver_has_reaction is 0 again", "5*P*max_batch doubles", "Later calls allocate nothing", "Not built"):
        assert phrase in header, phrase
