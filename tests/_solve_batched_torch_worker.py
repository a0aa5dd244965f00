"""Subprocess worker: torch is imported FIRST, the batched solver works in place on [B, N, N] float64 torch CUDA tensors on
a non-default torch stream (torch.cuda.current_stream()): N = 128 (direct pointers) and N = 257 (odd instances are only
8-byte aligned: the staging path), checked bit for bit against single solves of each instance."""
import os
import sys

import torch  # first, on purpose

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np  # noqa: E402
import _solve_ref as ref  # noqa: E402
import multigrid_poisson_solver_amd as mg  # noqa: E402

mg.init(0)
opts = dict(rtol=1e-10, max_cycles=12)
for N in (128, 257):
    B = 3
    probs = [ref.random_problem(N, 500 + i) for i in range(B)]
    tF = torch.from_numpy(np.stack([p[0] for p in probs])).cuda()
    tU = torch.from_numpy(np.stack([p[1] for p in probs])).cuda()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        tU.mul_(1.0)   # queued on the side stream ahead of the solve
        out, infos = mg.solve_batched(tF, tU, **opts)
        assert out is tU
    st.synchronize()
    got = tU.cpu().numpy()
    for i, (F, U0) in enumerate(probs):
        want_U, want = mg.solve(F, U0, **opts)
        assert np.array_equal(got[i].view(np.uint64), want_U.view(np.uint64)), f"N={N} instance {i} differs"
        assert infos[i]["history"] == want["history"] and infos[i]["cycles"] == want["cycles"]
    # one shared (N, N) F tensor for every instance
    tU2 = torch.from_numpy(np.stack([p[1] for p in probs])).cuda()
    with torch.cuda.stream(st):
        mg.solve_batched(tF[0].clone(), tU2, **opts)
    st.synchronize()
    for i in range(B):
        want_U, _ = mg.solve(probs[0][0], probs[i][1], **opts)
        assert np.array_equal(tU2[i].cpu().numpy().view(np.uint64), want_U.view(np.uint64)), f"N={N} shared F {i}"
assert mg.lib().mg_get_stream() != st.cuda_stream, "the engine stream was not restored"
mg.finalize()
print("SOLVE_BATCHED_TORCH OK")
