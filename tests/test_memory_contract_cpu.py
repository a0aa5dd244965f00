"""Host-side tests of the guard-band harness (tests/_guard.py): block layout and alignment in both placements, band
width, and the read-only table against the prototypes of include/mg_hip.h -- a new entry point that takes a device
array and has no row fails here."""
import os

import numpy as np
import pytest

import _guard

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mg_hip.h")

# prototypes with a double* / float* argument that are NOT device-array operators of the memory contract, and why
EXEMPT = {
    "mg_free": "allocator", "mg_free_f32": "allocator",
    "mg_upload": "the harness's own transport (host <-> device copies)", "mg_download": "transport",
    "mg_upload_f32": "transport", "mg_download_f32": "transport",
    "mg_restriction_table": "host arrays only", "mg_prolongation_table": "host arrays only",
    "mg_cycle_refinement_errors": "host array", "mg_slab_refinement_errors": "host array",
    "mg_slab_gather_U": "host array", "mg_print2File": "CSV writer (reads a device array into a file)",
}


def prototypes():
    with open(HEADER) as f:
        return _guard.parse_prototypes(f.read())


@pytest.mark.parametrize("itemsize", [4, 8])
@pytest.mark.parametrize("placement", _guard.PLACEMENTS)
@pytest.mark.parametrize("shapes", [[4], [5, 5, 5], [17, 8, (1, 2)], [65, 32], [257, 128, 257], [2049, 1024, 2049], [8192, 4096]])
def test_layout(shapes, placement, itemsize):
    offsets, total, guard = _guard.layout(shapes, itemsize, placement)
    sizes = [int(np.prod(_guard._shape(s))) for s in shapes]
    Nmax = max(max(_guard._shape(s)) for s in shapes)
    assert guard >= 8 * Nmax + 1024
    end = 0
    for off, n in zip(offsets, sizes):
        start = off * itemsize
        assert start % 16 == 0                                   # the alignment the contract gives
        assert start % 4096 == (0 if placement == "page" else 16)  # ... and, for odd16, nothing more
        assert off - end >= guard                                # band in front
        end = off + n
    assert total - end >= guard                                  # band behind the last array
    assert total * itemsize % 16 == 0


def test_odd16_is_two_doubles_past_512():
    offsets, _, _ = _guard.layout([5, 5], 8, "odd16")
    assert all(o % 512 == 2 for o in offsets)


def test_bad_placement_is_refused():
    with pytest.raises(ValueError):
        _guard.layout([8], 8, "anywhere")


def test_header_parses():
    p = prototypes()
    assert p["mg_getResidual"] == [("int", "N"), ("double", "L"), ("double *", "U"), ("double *", "F"), ("double *", "D")]
    assert ("const double *", "U_in") in p["mg_smooth_pp"]
    assert p["mg_checksum"][-1] == ("uint64_t *", "out")
    assert ("const double *const *", "F_dev") in p["mg_batch_solver_solve"]


def _is_pointer(typ):
    return "*" in typ


def test_table_covers_every_device_pointer_of_every_listed_prototype():
    p = prototypes()
    for name, row in _guard.CONTRACT.items():
        assert name in p, f"{name} is not declared in mg_hip.h"
        pointers = [(t, a) for t, a in p[name] if _is_pointer(t) and (name, a) not in _guard.HOST_POINTERS]
        assert [a for _, a in pointers] == list(row), f"{name}: table {list(row)} vs prototype {pointers}"
        for t, a in pointers:
            assert row[a] in ("in", "out", "inout", "clobber")
            if t.startswith("const"):
                # a const argument is read only; the one documented exception is U_in of mg_smooth_pp
                assert row[a] == "in" or (name, a) == ("mg_smooth_pp", "U_in"), f"{name}({a}) is const but listed {row[a]}"
    assert [k for k, r in _guard.CONTRACT.items() if "clobber" in r.values()] == ["mg_smooth_pp"]


def test_every_entry_point_with_a_device_array_has_a_row():
    for name, args in prototypes().items():
        if any(("double *" in t or "float *" in t) and "mg_" not in t for t, _ in args):
            assert name in _guard.CONTRACT or name in EXEMPT, f"{name} takes an array and has no row in _guard.CONTRACT"


def test_where_names_row_and_column():
    class FakeBlock:
        _where = _guard.GuardedBlock._where
    b = FakeBlock()
    offsets, total, _ = _guard.layout([10, 10], 8, "page")
    b.views = [type("V", (), dict(offset=o, size=100, shape=(10, 10), index=i))() for i, o in enumerate(offsets)]
    assert "array 0 (10, 10): row 10, column 0" in b._where(offsets[0] + 100)   # one row past the end
    assert "array 1 (10, 10): row -1, column 9" in b._where(offsets[1] - 1)
