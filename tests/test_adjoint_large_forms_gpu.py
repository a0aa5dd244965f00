"""The non-temporal form of the coefficient-gradient kernel (include/mg_adjoint.h; even N >= 4096: column pairs, 16-byte
accesses, non-temporal stores of gA), bit for bit against the restatement -- the N = 4096 case of tests/test_adjoint_gpu.py's
kernel test, in a file of its own because of its size (three 128 MiB arrays)."""
import pytest

import test_adjoint_gpu as t

pytestmark = pytest.mark.gpu


def test_point_kernels_non_temporal_form(mg):
    t.check_point_kernels(mg, 4096)
