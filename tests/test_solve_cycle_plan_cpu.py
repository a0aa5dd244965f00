"""The recorded V-cycle of the residual-tolerance solvers (mg_solve_cycle_describe, host only): the same
launches on the same fields as the functions it replaced (tests/_solve_cycle_ref.py), table slots that the batched
executor can rely on, and no step that overwrites a field still in use.  No GPU, no mg_init."""
import itertools
import os

import numpy as np
import pytest

import _solve_cycle_ref as ref


@pytest.fixture(scope="module")
def m():
    import multigrid_poisson_solver_amd as m
    if not os.path.exists(m.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    m.load_library()
    return m


def fusable_patterns(nl):
    """every combination of bits up to four levels; all-true, all-false and alternating at eleven"""
    n = nl - 1
    if nl <= 4:
        return [list(b) for b in itertools.product((0, 1), repeat=n)]
    return [[1] * n, [0] * n, [i % 2 for i in range(n)]]


def all_cases():
    for nl in (2, 3, 4, 11):
        tops = sorted({t for t in (0, 1, nl - 2) if 0 <= t <= nl - 2})   # (a cycle has at least two levels: top <= nl - 2)
        for pre, post, top in itertools.product(range(1, 5), range(1, 5), tops):
            for with_coef in (0, 1):
                yield dict(nl=nl, pre=pre, post=post, top=top, fused=0, with_coef=with_coef, down=None, up=None)
            for down, up in itertools.product(fusable_patterns(nl), repeat=2):
                yield dict(nl=nl, pre=pre, post=post, top=top, fused=1, with_coef=0, down=down, up=up)


@pytest.fixture(scope="module")
def described(m):
    """every case once: (case, steps as the restatement writes them, slots)"""
    out = []
    for c in all_cases():
        rec = m.solve_cycle(c["nl"], c["pre"], c["post"], c["top"], c["fused"], c["down"], c["up"], c["with_coef"])
        assert rec.shape[1] == 16
        steps = [tuple(int(v) for v in r[:5]) + tuple((int(r[5 + 2 * i]), int(r[6 + 2 * i])) for i in range(5)) for r in rec]
        out.append((c, steps, [int(r[15]) for r in rec]))
    assert len(out) > 4000
    return out


def test_sequence_equals_the_replaced_functions(described):
    for c, steps, _ in described:
        want = (ref.fused_cycle(c["nl"], c["pre"], c["post"], c["top"], c["down"], c["up"]) if c["fused"]
                else ref.ops_cycle(c["nl"], c["pre"], c["post"], c["top"], c["with_coef"]))
        assert steps == want, c


def test_slots_are_consistent_dense_and_no_more_than_the_tables_before(described):
    for c, steps, slots in described:
        roles = [s[5:] for s in steps]
        # equal roles <=> equal slot: the pairs (roles, slot) are a one-to-one map between the distinct roles and the slots
        assert len(set(zip(roles, slots))) == len(set(roles)) == len(set(slots)), (c, roles, slots)
        n_slots = max(slots)
        assert sorted(set(slots)) == list(range(1, n_slots + 1)), c
        # table 0 is the norm's: the upload is n_slots + 1 tables, the parent's n_tables / n_tables_vc
        before = ref.n_tables(c["nl"]) if c["fused"] else ref.n_tables_vc(c["nl"])
        assert n_slots + 1 <= before, (c, n_slots, before)


def test_no_step_overwrites_a_field_in_use(described):
    """A symbolic walk: per level the field holding its live iterate and its source, and the residual awaiting its
    restriction.  Every step reads the live fields of its level and writes a field that holds nothing live."""
    for c, steps, _ in described:
        top, last = c["top"], c["nl"] - 1
        U0, F0 = (ref.F_U0, top), (ref.F_F0, top)
        iterate, source, resid = {top: U0}, {top: F0}, None
        for n, (kind, l, _, d_sign, transfer, inp, F, coarse, out, Fc) in enumerate(steps):
            live = set(iterate.values()) | set(source.values()) | ({resid} if resid else set())
            what = (c, n, steps[n])
            assert out != ref.NONE and out not in live and out not in (inp, coarse), what
            if kind in (ref.SWEEP, ref.NODE, ref.RESIDUAL, ref.COARSE):
                assert F == source[l], what
            if kind in (ref.SWEEP, ref.RESIDUAL, ref.COARSE):
                assert coarse == ((ref.F_COEF, l) if c["with_coef"] else ref.NONE), what
            if kind == ref.SWEEP or (kind == ref.NODE and not (transfer and d_sign > 0)):
                assert inp == iterate.get(l, ref.NONE), what            # (no iterate yet: the zero start)
                iterate[l] = out
                if kind == ref.NODE and transfer:
                    assert Fc != ref.NONE and Fc not in live and Fc != out, what
                    source[l + 1] = Fc
            elif kind == ref.RESIDUAL:
                assert inp == iterate[l] and resid is None, what
                resid = out
            elif kind == ref.RESTRICT:
                assert inp == resid, what
                source[l + 1], resid = out, None
            elif kind == ref.COARSE:
                assert l == last and inp == ref.NONE and l not in iterate, what
                iterate[l] = out
            elif kind in (ref.PROLONG_ADD, ref.NODE):
                assert inp == iterate[l] and coarse == iterate[l + 1], what
                iterate[l] = out
                del iterate[l + 1], source[l + 1]
            else:
                assert kind == ref.COPY and n == len(steps) - 1 and inp == iterate[top] and out == U0, what
                iterate[top] = out
        assert iterate == {top: U0} and source == {top: F0} and resid is None, c
        written = [s for s in steps if s[0] != ref.COPY][-1][8]
        assert (steps[-1][0] == ref.COPY) == (written != U0), c


def test_describe_refuses_bad_arguments(m):
    lib = m.load_library()
    lib.mg_set_abort_on_error(0)   # (the library's default is the reference's, print and exit; init() sets the same 0)
    try:
        assert lib.mg_solve_cycle_describe(1, 1, 1, 0, 0, None, None, 0, None, 0) == -1
        assert lib.mg_solve_cycle_describe(3, 1, 1, 2, 0, None, None, 0, None, 0) == -1
        assert lib.mg_solve_cycle_describe(3, 1, 1, 0, 1, None, None, 0, None, 0) == -1
        assert lib.mg_last_error() != 0
    finally:
        lib.mg_clear_error()
    some = np.zeros((2, 16), dtype=np.int32)   # fewer records than steps: the count is still the whole cycle's
    assert lib.mg_solve_cycle_describe(3, 1, 1, 0, 0, None, None, 0, some.ctypes.data, 2) == len(ref.ops_cycle(3, 1, 1, 0, 0))
