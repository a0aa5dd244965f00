"""Child process of test_solve_gpu.py::test_product_size_two_cycles: two solve cycles at N x N (default options) on
the getSource problem with U = 0, with the library's own thresholds (the caller removed the MG_* overrides of the test
suite).  Prints the final U as a 128-bit device checksum and the residual history."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import multigrid_poisson_solver_amd as mg

mg.init(0)
N = int(sys.argv[1])
F = mg.getSource(N)
U = mg.DeviceGrid.zeros((N, N))
s = mg.Solver(N, 1.0, rtol=0.0, atol=0.0, max_cycles=2)
_, info = s.solve(F, U)
s.close()
out = (C.c_uint64 * 2)()
mg.lib().mg_checksum(U.ptr, N * N, out)
print("SOLVE_BIG " + json.dumps({"N": N, "sum": [int(out[0]), int(out[1])], "history": info["history"],
                                  "device_ms": info["device_ms"]}), flush=True)
U.free()
F.free()
mg.finalize()
