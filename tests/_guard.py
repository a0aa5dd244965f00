"""Guard-band harness of the memory-contract tests (tests/test_memory_contract_gpu.py).  TEST INFRASTRUCTURE.

A GuardedBlock is ONE mg_alloc (or mg_alloc_f32) block that holds the arrays of a call one after the other, each with
a guard band in front of it and behind it.  A stray access of a kernel therefore stays inside memory the process owns
(nothing can fault) and is seen afterwards: the bands are filled with all-ones bytes -- 0xFFFFFFFFFFFFFFFF, a NaN as fp64
and as two fp32, with a payload no arithmetic produces (hardware NaNs are 0x7FF8... / 0xFFF8... or carry an input's
payload on) -- so a stray STORE changes a band (even a store of a NaN does), and a CONSUMED out-of-window read poisons
the output, which the bit comparison of the calling test then sees.  check() compares by bits: every band, and every
array the caller declared read-only for the call.

Guard width: at least 8*N + 1024 elements on each side (N the largest side in the block).  The bound comes from the
kernels, not from a measurement: none indexes further than PR = 4 / ROWS_PB = 4 rows (mg_kernels.hip, mg_solve_kernels.hip),
S + 2 <= 6 halo rows (mg_stream_impl.h) or one strip of 64*4 columns past the edge of its window; 8 rows and 1024
elements cover each of them with room to spare.

Two placements: "page" -- every array starts on a multiple of 4 KiB, what hipMalloc gives; "odd16" -- every array
starts 16 bytes past a multiple of 4 KiB (2 doubles mod 512): 16-byte aligned, the alignment mg_alloc guarantees and the
solvers demand, and nothing more.  A kernel that silently assumes more must show as wrong bits."""
import ctypes as C

import numpy as np

PATTERN = 0xFFFFFFFFFFFFFFFF
PAGE = 4096
PLACEMENTS = ("page", "odd16")
DOWNLOAD_MAX_N = 2048   # up to here bands and inputs are downloaded and compared with numpy; above: mg_checksum


def guard_elems(N):
    """the least guard width (elements) for arrays of side N"""
    return 8 * int(N) + 1024


def _shape(s):
    return (int(s), int(s)) if isinstance(s, (int, np.integer)) else tuple(int(v) for v in s)


def layout(shapes, itemsize, placement):
    """Element offsets of the arrays inside the block, and the block's size in elements (pure host arithmetic).
    Returns (offsets, total, guard): every array is preceded and followed by at least `guard` elements of band."""
    if placement not in PLACEMENTS:
        raise ValueError(f"placement {placement!r} (have {PLACEMENTS})")
    shapes = [_shape(s) for s in shapes]
    guard = guard_elems(max(max(s) for s in shapes))
    skew = 0 if placement == "page" else 16
    offsets, pos = [], 0   # pos: first byte free after the previous array
    for s in shapes:
        start = pos + guard * itemsize
        start = (start + PAGE - 1) // PAGE * PAGE + skew
        offsets.append(start // itemsize)
        pos = start + int(np.prod(s)) * itemsize
    total = pos + guard * itemsize
    total = (total + 15) // 16 * 16
    return offsets, total // itemsize, guard


class GuardView:
    """One array of a GuardedBlock: what the wrappers of multigrid_poisson_solver_amd take where they take a
    DeviceGrid (they use .ptr only)."""

    def __init__(self, block, index, offset, shape):
        self.block, self.index, self.offset = block, index, offset
        self.shape = shape
        self.size = int(np.prod(shape))
        self.ptr = block.ptr + offset * block.itemsize

    @property
    def N(self):
        return self.shape[0]

    def upload(self, a):
        b = self.block
        a = np.ascontiguousarray(a, dtype=b.dtype)
        assert a.size == self.size, (a.shape, self.shape)
        (b.lib.mg_upload if b.itemsize == 8 else b.lib.mg_upload_f32)(self.ptr, a.ctypes.data, a.size)
        b.mg._check()
        return self

    def poison(self):
        """all-ones bytes over the array: an output no element of which the call may leave unwritten"""
        ones = np.full(self.size, PATTERN if self.block.itemsize == 8 else 0xFFFFFFFF, dtype=np.uint64 if self.block.itemsize == 8 else np.uint32)
        return self.upload(ones.view(self.block.dtype))

    def fill_uniform(self, seed):
        assert self.block.itemsize == 8
        self.block.lib.mg_fill_uniform(self.ptr, self.size, seed)
        self.block.mg._check()
        return self

    def to_host(self):
        b = self.block
        out = np.empty(self.shape, dtype=b.dtype)
        (b.lib.mg_download if b.itemsize == 8 else b.lib.mg_download_f32)(out.ctypes.data, self.ptr, self.size)
        b.mg._check()
        return out

    def checksum(self):
        return self.block._checksum(self.offset, self.size)

    def free(self):   # (the block owns the memory)
        pass


class GuardedBlock:
    def __init__(self, mg, shapes, dtype=np.float64, placement="page"):
        self.mg, self.lib = mg, mg.lib()
        self.dtype = np.dtype(dtype)
        self.itemsize = self.dtype.itemsize
        assert self.itemsize in (4, 8)
        self.placement = placement
        self.shapes = [_shape(s) for s in shapes]
        self.offsets, self.total, self.guard = layout(self.shapes, self.itemsize, placement)
        # (mg_checksum reads doubles: fp32 blocks, whose arrays may hold an odd number of floats, are always downloaded)
        self.big = max(max(s) for s in self.shapes) > DOWNLOAD_MAX_N and self.itemsize == 8
        self.ptr = (self.lib.mg_alloc if self.itemsize == 8 else self.lib.mg_alloc_f32)(self.total)
        mg._check()
        if not self.ptr:
            raise mg.MGError("mg_alloc returned NULL")
        assert self.ptr % 256 == 0
        self.views = [GuardView(self, i, o, s) for i, (o, s) in enumerate(zip(self.offsets, self.shapes))]
        # bands: [begin, end) in elements -- everything that is not an array
        edges = [0]
        for v in self.views:
            edges += [v.offset, v.offset + v.size]
        edges.append(self.total)
        self.bands = [(edges[2 * i], edges[2 * i + 1]) for i in range(len(self.views) + 1)]
        for lo, hi in self.bands:
            if self.itemsize == 8:
                pat = np.full(hi - lo, PATTERN, dtype=np.uint64)
                self.lib.mg_upload(self.ptr + lo * 8, pat.ctypes.data, pat.size)
            else:
                pat = np.full(hi - lo, 0xFFFFFFFF, dtype=np.uint32)
                self.lib.mg_upload_f32(self.ptr + lo * 4, pat.ctypes.data, pat.size)
        mg._check()
        self._readonly, self._before = [], None

    def __iter__(self):
        return iter(self.views)

    def __getitem__(self, i):
        return self.views[i]

    # ---------------------------------------------------------------- state before / after
    def _checksum(self, offset, count):
        """mg_checksum over `count` doubles from `offset`"""
        assert self.itemsize == 8
        n = count
        out = (C.c_uint64 * 2)()
        self.lib.mg_checksum(self.ptr + offset * self.itemsize, n, out)
        self.mg._check()
        return int(out[0]), int(out[1])

    def _raw(self, lo, hi):
        """elements [lo, hi) of the block as bit patterns (uint64, or uint32 for fp32 blocks)"""
        out = np.empty(hi - lo, dtype=np.uint64 if self.itemsize == 8 else np.uint32)
        (self.lib.mg_download if self.itemsize == 8 else self.lib.mg_download_f32)(out.ctypes.data, self.ptr + lo * self.itemsize, hi - lo)
        self.mg._check()
        return out

    def expect_readonly(self, *views):
        """Declare the arrays the coming call may only read, and record them (and, for large blocks, the bands)."""
        self._readonly = list(views)
        if self.big:
            self._before = dict(bands=[self._checksum(lo, hi - lo) for lo, hi in self.bands],
                                arrays=[v.checksum() for v in views])
        else:
            self._before = dict(arrays=[self._raw(v.offset, v.offset + v.size) for v in views])
        return self

    def _where(self, e):
        """element e of the block as (array index, row, column) relative to the nearest array"""
        best = min(self.views, key=lambda v: 0 if v.offset <= e < v.offset + v.size else
                   min(abs(e - v.offset), abs(e - (v.offset + v.size - 1))))
        rel = e - best.offset
        width = best.shape[-1]
        return f"array {best.index} {best.shape}: row {rel // width}, column {rel % width}"

    def check(self, what=""):
        """every guard band unchanged, every array declared read-only unchanged -- by bits"""
        if self._before is None:
            self.expect_readonly()
        full = np.uint64(PATTERN) if self.itemsize == 8 else np.uint32(0xFFFFFFFF)
        if self.big:
            for i, ((lo, hi), was) in enumerate(zip(self.bands, self._before["bands"])):
                now = self._checksum(lo, hi - lo)
                assert now == was, f"{what}: guard band {i} (elements {lo}..{hi}, {self.placement}) changed: checksum {was} -> {now}"
            for v, was in zip(self._readonly, self._before["arrays"]):
                now = v.checksum()
                assert now == was, f"{what}: read-only array {v.index} {v.shape} changed: checksum {was} -> {now}"
        else:
            for i, (lo, hi) in enumerate(self.bands):
                raw = self._raw(lo, hi)
                bad = np.flatnonzero(raw != full)
                if bad.size:
                    e = lo + int(bad[0])
                    raise AssertionError(f"{what}: guard band {i} ({self.placement}) written at {bad.size} elements, first at "
                                         f"{self._where(e)} (bits {int(raw[bad[0]]):#x})")
            for v, was in zip(self._readonly, self._before["arrays"]):
                now = self._raw(v.offset, v.offset + v.size)
                bad = np.flatnonzero(now != was)
                if bad.size:
                    e = int(bad[0])
                    raise AssertionError(f"{what}: read-only array {v.index} {v.shape} changed at {bad.size} elements, first at "
                                         f"row {e // v.shape[-1]}, column {e % v.shape[-1]}")
        self._before = None
        self._readonly = []

    def free(self):
        if self.ptr:
            (self.lib.mg_free if self.itemsize == 8 else self.lib.mg_free_f32)(self.ptr)
        self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def block(mg, shapes, placement, dtype=np.float64):
    return GuardedBlock(mg, shapes, dtype, placement)


# -------------------------------------------------------------------------------------------------
# the read-only table: for every entry point of include/mg_hip.h that takes a device array, each device-pointer
# argument in the prototype's order with what the header says of it --
#   "in":      read only (const in the prototype, or the header's comment says "read only")
#   "out":     written by the call
#   "inout":   read and written
#   "clobber": an input the header allows the call to overwrite as scratch (nothing asserted on its contents)
# (host pointers -- error of mg_doSmoothing, error_host, out[2] of mg_checksum -- are not device arrays)
# -------------------------------------------------------------------------------------------------
CONTRACT = {
    "mg_copy": {"dst_dev": "out", "src_dev": "in"},
    "mg_fill_zero": {"dev": "out"},
    "mg_negate": {"D": "inout"},
    "mg_getSource": {"F": "out"},
    "mg_getAnalytic": {"U": "out"},
    "mg_analyticError": {"U": "in"},
    "mg_getResidual": {"U": "in", "F": "in", "D": "out"},
    "mg_doGridAddition": {"U1": "inout", "U2": "in"},
    "mg_doSmoothing": {"U": "inout", "F": "in"},
    "mg_doExactSolver": {"U": "out", "F": "in"},
    "mg_doRestriction": {"U_f": "in", "U_c": "out"},
    "mg_doProlongation": {"U_c": "in", "U_f": "inout"},
    "mg_smooth_pp": {"U_in": "clobber", "U_out": "out", "F": "in", "error_dev": "out", "D_out": "out"},
    "mg_smooth_restrict": {"U_in": "in", "U_out": "out", "F": "in", "error_dev": "out", "F_c": "out"},
    "mg_prolong_smooth": {"U_c": "in", "U_in": "in", "U_out": "out", "F": "in", "error_dev": "out"},
    "mg_smooth_restrict_f32": {"U_in": "in", "U_out": "out", "F": "in", "error_dev": "out", "F_c": "out"},
    "mg_prolong_smooth_f32": {"U_c": "in", "U_in": "in", "U_out": "out", "F": "in", "error_dev": "out"},
    "mg_to_f32": {"dst_dev": "out", "src_dev": "in"},
    "mg_to_f64": {"dst_dev": "out", "src_dev": "in"},
    "mg_prolongAdd": {"U_c": "in", "U_f_in": "in", "U_f_out": "out"},
    "mg_restrict_signed": {"U_f": "in", "U_c": "out"},
    "mg_fill_uniform": {"dst": "out"},
    "mg_checksum": {"src": "in"},
    "mg_solver_solve": {"F_dev": "in", "U_dev": "inout"},
    "mg_batch_solver_solve": {"F_dev": "in", "U_dev": "inout"},
}
HOST_POINTERS = {("mg_doSmoothing", "error"), ("mg_analyticError", "error_host"), ("mg_checksum", "out"),
                 ("mg_solver_solve", "s"), ("mg_solver_solve", "out"), ("mg_batch_solver_solve", "s"),
                 ("mg_batch_solver_solve", "out"), ("mg_batch_solver_solve", "stats")}


def parse_prototypes(header_text):
    """{function name: [(type, argument name)]} of every prototype in the header that has a pointer argument"""
    import re
    text = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b([A-Za-z_][\w \*]*?)\b(mg_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        name, args = m.group(2), m.group(3).strip()
        if args in ("", "void"):
            continue
        parsed = []
        for a in args.split(","):
            a = " ".join(a.split())
            mm = re.match(r"(.*?)(\w+)(\[\d*\])?$", a)
            typ, arg = mm.group(1).strip(), mm.group(2)
            if mm.group(3):
                typ += " *"
            parsed.append((typ, arg))
        out[name] = parsed
    return out
