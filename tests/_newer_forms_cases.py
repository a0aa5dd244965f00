"""The case tables of tests/test_newer_forms_gpu.py, shared with tests/test_newer_forms_cpu.py, which checks on the CPU what
the GPU cases rest on: the gap condition of every eigen case and the qualification of every FMG seed.  TEST INFRASTRUCTURE."""
import numpy as np

import _eigs_ref as er

RTOL = 1e-8        # the eigen-solver's default
MAX_ITERS = 60     # and its cap: every case below converges within half of it

# (profile, axis) of _eigs_ref.layered: "one" once, each layered profile in both orientations -- a kernel that mixes rows and
# columns up passes "one" and fails one orientation of the other two
EIG_FIELDS = [("one", "cols"), ("smooth", "cols"), ("smooth", "rows"), ("jump", "cols"), ("jump", "rows")]

# N -> [(k, guard)].  p = k + guard; the basis holds p, 2p and 3p fields (the first step, the step after a restart, every
# other step), so the rotation runs the buckets
#   p = 3:   M = 3, 6, 12   the pair form of the rotation at even N           (1, 2) at 512, 514
#   p = 6:   M = 6, 12, 18  pair form, then the column form at a pair size    (4, 2) at 512; odd N: 513
#   p = 8:   M = 12, 18, 24 pair form, then both column buckets               (4, 4) at 514
#   p = 12:  M = 12, 24, 36 the full block, at one size only                  (8, 4) at 512
# k in {1, 4, 8}: on "one" the pairs lam_12 = lam_21, lam_13 = lam_31, lam_23 = lam_32, lam_14 = lam_41 are degenerate,
# and k = 2, 3, 5, 6, 7, 9 would split one (test_newer_forms_cpu.py holds the gap condition for every case)
EIG_BLOCKS = {512: [(1, 2), (4, 2), (8, 4)], 514: [(1, 2), (4, 4)], 513: [(4, 2)]}
# 1026 -> 513 -> 256: one solve, the jump along the columns, the smallest block (its longdouble checks cost four times 512's)
EIG_CASES = [(N, name, axis, k, guard) for N, blocks in EIG_BLOCKS.items() for k, guard in blocks for name, axis in EIG_FIELDS]
EIG_CASES.append((1026, "jump", "cols", 1, 2))

# iterations of the numpy restatement _eigs_ref.solve(seed=3) on the CPU, the evidence that each case converges inside
# MAX_ITERS / 2 = 30 (the engine's own Jacobi routine may differ by one or two: _eigs_ref's docstring).  (N, k, guard) ->
# the counts over EIG_FIELDS; 5 to 70 s each on the CPU, so they are recorded here, not re-run by a test.  The MI355X took
# the same number of iterations in all 31 cases.
RESTATEMENT_ITERS = {(512, 1, 2): [11, 11, 12, 16, 16], (512, 4, 2): [17, 18, 19, 17, 17], (512, 8, 4): [16, 17, 16, 18, 18],
                     (514, 1, 2): [11, 12, 13, 16, 17], (514, 4, 4): [14, 16, 15, 16, 15], (513, 4, 2): [17, 18, 17, 18, 18],
                     (1026, 1, 2): [18]}    # (1026: jump / cols alone)


def gap_left_out(cases=None, rtol=RTOL):
    """the cases whose k-th gap does not exceed 4*rtol*sqrt(sum_{i<k} lam_i^2) on the separated reference: a converged
    solve has ||R||_F at most rtol*sqrt(sum lam_i^2), so on every other case the quadratic bound is asserted"""
    out = []
    for N, name, axis, k, guard in (EIG_CASES if cases is None else cases):
        lam = er.separated_eigenvalues(name, N, 1.0, 13)
        if not lam[k] - lam[k - 1] > 4.0 * rtol * float(np.sqrt(np.sum(lam[:k] ** 2))):
            out.append((N, name, axis, k, guard))
    return out


# whole FMG solves whose hierarchy has an even level with an odd source: 514 -> 257 -> 128 ... and 1026 -> 513 -> 256 ...
# (N, fmg, shift, seed); two cycles each.  The seeds qualify on the restatement alone (test_newer_forms_cpu.py)
SEED_FMG = {514: 7514, 1026: 8026}
FMG_CASES = [(514, 1, 0.0), (514, 1, 1e2), (514, 2, 0.0), (514, 2, 1e2), (1026, 1, 0.0), (1026, 1, 1e2)]
FMG_CYCLES = 2
