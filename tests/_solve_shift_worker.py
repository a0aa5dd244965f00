"""Subprocess worker of test_solve_shift_gpu.py.
  fresh | refused: one shifted Solver solve and one shifted BatchSolver solve, printed as digests of U and history; in
      `refused` every refused creation (shift = -1, NaN, inf, from both creators) comes first, each followed by the solves.
  torch: torch imported FIRST, a shifted solve in place on float64 CUDA tensors on a side stream against the restatement."""
import hashlib
import os
import sys

mode = sys.argv[1]
if mode == "torch":
    import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
os.environ.setdefault("OMP_NUM_THREADS", "4")
import numpy as np  # noqa: E402
import _solve_ref as ref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
N, SIGMA = 129, 1e4
F, U0 = ref.random_problem(N, 21)


def digests():
    opts = dict(rtol=1e-10, max_cycles=12, shift=SIGMA)
    U, info = mg.solve(F, U0, **opts)
    Us, infos = mg.solve_batched(np.stack([F, F]), np.stack([U0, 2 * U0]), **opts)
    h = hashlib.sha256()
    for a in (U, Us, np.array(info["history"]), np.array(infos[0]["history"]), np.array(infos[1]["history"])):
        h.update(np.ascontiguousarray(a).tobytes())
    assert np.array_equal(U.view(np.uint64), Us[0].view(np.uint64)) and info["converged"]
    return h.hexdigest()


if mode in ("fresh", "refused"):
    got = []
    if mode == "refused":
        for bad in (-1.0, float("nan"), float("inf")):
            for make in (lambda: mg.Solver(N, 1.0, shift=bad), lambda: mg.BatchSolver(N, 1.0, max_batch=2, shift=bad)):
                try:
                    make()
                except mg.MGError as e:
                    assert "[2]" in str(e), e
                else:
                    raise SystemExit(f"shift = {bad} was accepted")
                got.append(digests())
        assert len(set(got)) == 1, got
    else:
        got.append(digests())
    mg.finalize()
    print(f"SOLVE_SHIFT {mode} {got[0]}")
else:
    import _oracle  # noqa: E402
    import _solve_shift_ref as sref  # noqa: E402
    orc = _oracle.Oracle()
    tF, tU = torch.from_numpy(F).cuda(), torch.from_numpy(U0).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        tU.mul_(1.0)   # queued on the side stream ahead of the solve
        out, info = mg.solve(tF, tU, rtol=0.0, max_cycles=2, shift=SIGMA)
        assert out is tU
    st.synchronize()
    want = U0
    for _ in range(2):
        want = sref.cycle(orc, F, want, shift=SIGMA)
    got = tU.cpu().numpy() + 0.0
    assert np.array_equal(got.view(np.uint64), (want + 0.0).view(np.uint64)), "shifted solve on torch tensors differs"
    assert info["cycles"] == 2
    tB = torch.from_numpy(np.stack([U0, U0])).cuda()
    outB, infos = mg.solve_batched(tF, tB, rtol=0.0, max_cycles=2, shift=SIGMA)
    assert np.array_equal((outB[1].cpu().numpy() + 0.0).view(np.uint64), (want + 0.0).view(np.uint64)), "batched torch solve differs"
    mg.finalize()
    print("SOLVE_SHIFT torch OK")
