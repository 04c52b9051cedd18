"""
Host side of the MI355X weight-application engine: ``libremap_hip.so``
(``include/remap_hip.h``; ``_abi.py`` is its ctypes mirror) loaded, the
device-resident plan and the launches.  The weight-generation wrappers live
in ``geometry.py`` and are re-exported at the end of this file.

This is the layer that replaces, for ``Remapper.remap_numpy``:

* ``remap_numpy.py:134-137`` -- ``RemapPlan.from_triplets`` (COO -> CSR on
  the device, cached on the Remapper where the reference caches ``_matrix``);
* ``remap_numpy.py:223-297`` -- ``remap_array`` (``_remap_numpy_array``):
  the permute/flatten and unflatten/unpermute steps become strides handed to
  the kernel, the SpMM + normalisation + masking is one fused HIP launch.

PyTorch is used for device memory, streams and (in ``parallel.py``)
``torch.distributed``; the arithmetic is in the HIP library.  There is no CPU
fallback: without the library or without a GPU every compute entry point
raises.
"""
import collections
import contextlib
import ctypes
import os

import numpy as np

from pyremap_amd import _abi, _build
from pyremap_amd._abi import (  # noqa: F401  (tests and tools read them here)
    EXPORTS, _ApplyArgs, _CSR, _Field, _LayersArgs, _LevelsArgs, _LimitArgs,
    _OverlapGeom, _OverlapGrid, _OverlapMesh, _OverlapPieces, _OverlapSide,
    _PlanInfo, _Schedule, _SgsArgs, _Strips, _VectorArgs)

MODE_RAW = 0
MODE_FRACB = 1
MODE_MASKED = 2
MODE_LAF = 3           # largest area fraction, for labels (pyremap_amd.laf)
# sub-grid statistics (pyremap_amd.rowstat); 4 to 7 are not assigned
MODE_MIN = 8
MODE_MAX = 9
MODE_VAR = 10
MODE_MEDIAN = 11
# class and bin area fractions (pyremap_amd.classfrac); 12 is not assigned
MODE_CLASSFRAC = 13
# the cotangent of the division, the first step of the adjoint apply
# (pyremap_amd.adjoint; cotangent_strided); 14 and 15 are not assigned
MODE_COTAN_FRACB = 16
MODE_COTAN_MASKED = 17
# one pass of a creeping fill over a grid's neighbour plan (pyremap_amd.fill;
# fill_tensor repeats it); 18 and 19 are not assigned
MODE_FILL_BEST = _abi.MODE_FILL_BEST
MODE_FILL_MEAN = _abi.MODE_FILL_MEAN
#: the modes that are a row pass over the plan's own CSR: no schedule, no
#: tune, no split, one device; what an error message calls each
_ROW_PASS_MODES = {MODE_LAF: 'largest area fraction',
                   MODE_MIN: 'a row statistic', MODE_MAX: 'a row statistic',
                   MODE_VAR: 'a row statistic',
                   MODE_MEDIAN: 'a row statistic',
                   MODE_CLASSFRAC: 'class fractions',
                   MODE_FILL_BEST: 'a fill', MODE_FILL_MEAN: 'a fill'}
#: what ``method=`` of a fill accepts (fill_tensor, Remapper.fill)
FILL_METHODS = {'nearest': MODE_FILL_BEST, 'mean': MODE_FILL_MEAN}
#: passes fill_tensor launches between two looks at the missing count
FILL_CHECK_EVERY = 4

FLAG_FMA = 1
FLAG_TUNE_HINT = 4
FLAG_TREE = 8
FLAG_CELL_MASKS = 16   # masked mode, a hint: validity is per source cell
FLAG_BATCH_MASKS = 32  # masked mode, a hint: the same mask in every batch

#: long rows apart (RemapPlan._split_long_rows): up to this many fields the
#: long rows run one wave per (row, few columns) -- family 9 -- beyond it on
#: the LDS-staged lanes-across-rows kernel (family 7)
LONG_WAVE_FIELDS = 16
#: long rows per workgroup (one wave each) of family 11 (spmm_longwave), which
#: takes the long rows' launch from LONG_WAVE_FIELDS + 1 to LONG_WAVE_MAX
#: fields; 0: family 7 there too.  1 deg -> 0.5 deg with pole caps, the long
#: rows' launch replayed, us, family 7 / family 11 with 4 / 6 / 8 rows:
#: K = 24 26.5 / 23.9 / 20.0 / 19.2, 64 26.2 / 23.4 / 19.8 / 19.1, 128 38.2 /
#: 28.3 / 27.4 / 36.3, 256 50.7 / 51.4 / 50.0 / 54.2, 512 61.3 / 98 / 95 / 107
LONG_WAVE_ROWS = 6
LONG_WAVE_MAX = 128
#: fields whose contiguous run behind the source axes is shorter than this
#: (and that come in several batches) take the lanes-across-rows kernels
CELL_MAX_RUN = 4

DTYPE_F64 = 0
DTYPE_F32 = 1

#: what ``reduce=`` accepts (layers_strided, Remapper.layers): REMAP_REDUCE_*
REDUCE = {'mean': 0, 'integral': 1}

ABI_VERSION = 31

#: readable pad entries kept behind col/val (remap_csr.csr_pad)
CSR_PAD = 8
#: LDS a workgroup of the lanes-across-rows kernel may take (kPatchLdsMax)
CELL_LDS_MAX = 160 * 1024
_LONG_TT = None   # (experiments: fields per lane of the long-row launch)
_LONG_WAVE_TT = None   # (tests: columns per wave of family 9, 0 = auto)
_CELL_TUNE = None      # (tools/tn_probe.py: [TT, one-chunk kernel?] of family 7)
_RUNS_TUNE = None      # (tools/runs_probe.py: the batch-at-a-time launch's tune)

#: what ``limiter=`` accepts (remap_tensor, Remapper.limiter)
LIMITERS = (None, 'clip', 'caas')


_lib = None


class EngineError(RuntimeError):
    """A failure reported by libremap_hip.so (message from the C side)."""


def library_path():
    return _build.LIB_PATH


def load_library():
    """
    Load ``libremap_hip.so``; build it first if it is missing and hipcc is
    available.  Raises if the library cannot be provided -- there is no other
    implementation to fall back to.
    """
    global _lib
    if _lib is not None:
        return _lib
    # torch brings its own HIP runtime (torch/lib/libamdhip64.so); the
    # library's RUNPATH names the system one.  Whichever is loaded first
    # serves the whole process, and a process with BOTH initialised sees "no
    # ROCm-capable device" from the second: torch first, always.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    path = _build.LIB_PATH
    if not os.path.exists(path):
        if _build.find_hipcc() is None:
            raise EngineError(
                f'{path} is missing and hipcc is not available to build it; '
                f'run `python -c "import __graft_entry__ as g; g.build()"` '
                f'on a machine with ROCm')
        _build.build_library()
    _lib = open_library(path)
    return _lib


def open_library(path):
    """
    ``ctypes.CDLL(path)``, checked against ``EXPORTS`` and the ABI version,
    with every entry point's prototype declared.  ``load_library`` keeps
    the one the package works with; a second library of the same ABI (the
    tests' wide-index build, ``_build.WIDE_LIB_PATH``) is opened with this and
    put in its place by setting ``engine._lib``.
    """
    lib = ctypes.CDLL(path)
    missing = [name for name in EXPORTS if not hasattr(lib, name)]
    if missing:
        raise EngineError(f'{path} lacks symbols {missing}')
    _abi.declare(lib)
    if lib.remap_abi_version() != ABI_VERSION:
        raise EngineError(
            f'{path} has ABI {lib.remap_abi_version()}, expected '
            f'{ABI_VERSION}; rebuild it')
    return lib


def _check(rc, what):
    if rc != 0:
        msg = load_library().remap_last_error().decode('utf-8', 'replace')
        raise EngineError(f'{what} failed ({rc}): {msg}')


def _torch():
    import torch
    return torch


def require_gpu():
    torch = _torch()
    if not torch.cuda.is_available():
        raise EngineError(
            'no HIP device is visible: the remapping engine runs on MI355X '
            'only (there is no CPU implementation in pyremap_amd)')
    load_library()
    return torch


def _stream_ptr(device):
    torch = _torch()
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


@contextlib.contextmanager
def _gpu_ms(torch, timing):
    """``timing['ms']``: the GPU time of the body, between an event recorded
    on the current stream on entry and one recorded on exit, which is waited
    for.  With ``timing`` None nothing is done at all: no event, no wait.  An
    exception of the body passes through and ``timing`` is not filled."""
    if timing is None:
        yield
        return
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    yield
    t1.record()
    t1.synchronize()
    timing['ms'] = t0.elapsed_time(t1)


# ---------------------------------------------------------------------------
# the plan: device-resident CSR + frac_b
# ---------------------------------------------------------------------------

class RemapPlan:
    """
    Device-resident weights of one mapping file (or of a row shard of it):
    what the reference keeps as ``remapper._matrix`` plus ``frac_b``.

    Attributes
    ----------
    n_a, n_b : int
        source size and number of destination rows HELD by this plan
    n_b_global : int
        destination size of the whole mapping
    row_offset : int
        global index of this plan's first row (0 unless sharded)
    rowptr, col, val, frac_b : torch.Tensor
        int64[n_b + 1], int32[nnz], float64[nnz], float64[n_b] on ``device``
    """

    def __init__(self, n_a, n_b, rowptr, col, val, frac_b, row_offset=0,
                 n_b_global=None):
        self.n_a = int(n_a)
        self.n_b = int(n_b)
        self.rowptr = rowptr
        self.frac_b = frac_b
        self.row_offset = int(row_offset)
        self.n_b_global = int(n_b if n_b_global is None else n_b_global)
        self.device = val.device
        torch = _torch()
        self.nnz = int(rowptr[-1]) if rowptr.numel() else 0
        #: col/val carry CSR_PAD readable entries behind the last one so a
        #: row's entries can be fetched 8 at a time (scalar-cache kernels)
        pad = int(val.shape[0]) - self.nnz
        if pad < CSR_PAD:
            col = torch.cat([col[:self.nnz], torch.zeros(
                CSR_PAD, dtype=col.dtype, device=col.device)])
            val = torch.cat([val[:self.nnz], torch.zeros(
                CSR_PAD, dtype=val.dtype, device=val.device)])
        self.csr_pad = int(val.shape[0]) - self.nnz
        self._col_padded = col
        self._val_padded = val
        self.col = col[:self.nnz]
        self.val = val[:self.nnz]
        #: entries of the longest row (kernel selection)
        self.max_row_nnz = int((rowptr[1:] - rowptr[:-1]).max()) \
            if self.n_b > 0 else 0
        self._touched = None
        self._arena = None
        self._row_last_col = None
        self._extent_cache = {}
        #: launch tuning used when a call passes none (set by auto_schedule)
        self.default_tune = None
        #: destination grid the schedules were built for (auto_schedule)
        self._grid_dims = None
        #: lazily built patch plan for the lanes-across-rows kernel that
        #: serves (Time, nCells)-like layouts (see cell_patches)
        self._cell = None
        #: lazily built small LDS patches for fields with short level runs
        #: (see run_patches)
        self._runs = None
        self._run_cells = None
        self._wave = None
        # schedule attributes are properties: every assignment invalidates
        # the prefilled argument block launches start from (_prefilled)
        self._sched_version = 0
        self._args_cache = {}
        #: optional LDS-staging schedule (see build_patches)
        self.patches = None
        #: optional row-group schedule (see build_groups)
        self.groups = None
        #: optional int32 permutation of the rows: the order in which work
        #: slots visit them (scheduling only; see set_row_order)
        self.row_order = None
        #: (short, long) sibling plans when a few rows hold a large share of
        #: the entries (see _split_long_rows); None otherwise
        self._split = None
        #: optional strip schedule of kernel family 8 (see build_strips)
        self.strips = None

    def _sched_property(name):   # noqa: N805 - class-body helper
        def get(self):
            return self.__dict__.get('_' + name)

        def put(self, value):
            self.__dict__['_' + name] = value
            self._sched_version += 1
        return property(get, put)

    patches = _sched_property('patches')
    groups = _sched_property('groups')
    strips = _sched_property('strips')
    row_order = _sched_property('row_order')
    del _sched_property

    def _prefilled(self, whole, cell=False):
        """
        A fresh ``remap_apply_args`` with everything that belongs to the plan
        filled in -- the CSR and, for a launch over the whole row range, the
        row order and the schedule that goes with it (``cell``: the patch
        plan of the lanes-across-rows kernel instead) -- copied from a block
        built once per schedule version (a Dataset of small variables is
        launch-overhead-bound: 2 launches per variable).
        """
        key = (whole, cell)
        hit = self._args_cache.get(key)
        if hit is not None and hit[0] == self._sched_version:
            return _ApplyArgs.from_buffer_copy(hit[1])
        args = _ApplyArgs()
        args.A = self._csr_struct()
        order = self.row_order
        if whole and cell:
            q = self._runs if cell == 'runs' else \
                self._run_cells if cell == 'run_cells' else \
                self._wave if cell == 'wave' else self._cell
            args.row_order = q['order'].data_ptr() \
                if q['order'] is not None else None
            args.patch_ptr = q['ptr'].data_ptr()
            args.patch_ucol = q['ucol'].data_ptr()
            args.patch_rowptr = q['rowptr'].data_ptr()
            args.patch_lidx = q['lidx'].data_ptr()
            args.patch_val = q['val'].data_ptr()
            args.patch_rows = q['rows']
            args.patch_umax = q['umax']
            args.patch_emax = q['emax']
            args.patch_row_bytes = q['row_bytes']
            args.n_patches = q['n']
            if q.get('ell_base') is not None:
                args.patch_ell_base = q['ell_base'].data_ptr()
        elif whole:
            # (a stored order permutes the whole row range: partial ranges
            # run without it, and without the schedules built on it)
            args.row_order = order.data_ptr() if order is not None else None

            def same_order(sched):
                return (order is None) == (sched['order'] is None) and (
                    order is None or
                    order.data_ptr() == sched['order'].data_ptr())
            patches = self.patches
            if patches is not None and same_order(patches):
                args.patch_ptr = patches['ptr'].data_ptr()
                args.patch_ucol = patches['ucol'].data_ptr()
                args.patch_rowptr = patches['rowptr'].data_ptr()
                args.patch_lidx = patches['lidx'].data_ptr()
                args.patch_val = patches['val'].data_ptr()
                args.patch_rows = patches['rows']
                args.patch_umax = patches['umax']
                args.patch_emax = patches['emax']
                args.patch_row_bytes = patches['row_bytes']
                args.n_patches = patches['n']
            groups = self.groups
            if groups is not None and same_order(groups):
                args.group_meta = groups['meta'].data_ptr()
                args.group_col = groups['col'].data_ptr()
                args.group_w = groups['w'].data_ptr()
                args.group_mask = groups['mask'].data_ptr()
                args.group_rid = groups['rid'].data_ptr()
                args.group_frac = groups['frac'].data_ptr()
                args.n_groups = groups['n']
                args.group_rows = groups['rows']
                share = groups.get('share')
                if share is not None:
                    args.share_meta = share['meta'].data_ptr()
                    args.share_col = share['col'].data_ptr()
                    args.share_mask = share['mask'].data_ptr()
                    args.share_waves = share['waves']
            if self.strips is not None:
                # (self-contained: its own row order and row ids)
                args.strips = ctypes.addressof(self.strips['struct'])
        self._args_cache[key] = (self._sched_version, bytes(args))
        return args

    # -- construction -------------------------------------------------------
    @classmethod
    def from_triplets(cls, row, col, S, frac_b, n_a, n_b, index_base=1,
                      device=None):
        """
        ``csr_matrix((S, (row - base, col - base)), shape=(n_b, n_a))`` on
        the device (``remap_numpy.py:134-137``).  ``row``/``col``/``S`` may
        be numpy arrays or torch tensors (host or device).
        """
        torch = require_gpu()
        lib = load_library()
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        device = torch.device(device)
        if n_a >= 2 ** 31 - 1 or n_b >= 2 ** 31 - 1:
            raise ValueError('the engine indexes cells with 32 bits: n_a and '
                             'n_b must stay below 2**31 - 1')

        def index32(v, name, extent):
            # Range-check BEFORE narrowing to int32: an int64 index of 2**31
            # or more would otherwise wrap into the valid range.
            t = torch.as_tensor(np.ascontiguousarray(v) if isinstance(
                v, np.ndarray) else v)
            if t.dtype != torch.int32 and t.numel():
                lo, hi = int(t.min()), int(t.max())
                if lo < index_base or hi >= extent + index_base:
                    bad = int(((t < index_base) |
                               (t >= extent + index_base)).sum())
                    raise ValueError(
                        f'{bad} mapping triplets have a {name} index outside '
                        f'[{index_base}, {extent + index_base - 1}]')
            return t.to(device=device, dtype=torch.int32)

        row_d = index32(row, 'row', n_b)
        col_d = index32(col, 'col', n_a)
        s_d = torch.as_tensor(np.ascontiguousarray(S) if isinstance(
            S, np.ndarray) else S).to(device=device, dtype=torch.float64)
        row_d, col_d, s_d = (row_d.contiguous(), col_d.contiguous(),
                             s_d.contiguous())
        nnz = int(s_d.shape[0])
        if row_d.shape[0] != nnz or col_d.shape[0] != nnz:
            raise ValueError('row, col and S must have the same length')
        frac_d = torch.as_tensor(
            np.ascontiguousarray(frac_b) if isinstance(frac_b, np.ndarray)
            else frac_b).to(device=device, dtype=torch.float64).contiguous()
        if frac_d.shape[0] != n_b:
            raise ValueError(f'frac_b has {frac_d.shape[0]} entries, '
                             f'expected n_b = {n_b}')
        with torch.cuda.device(device):
            nbytes = ctypes.c_size_t(0)
            _check(lib.remap_csr_from_coo_workspace(
                nnz, n_b, ctypes.byref(nbytes)),
                'remap_csr_from_coo_workspace')
            ws = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8,
                             device=device)
            rowptr = torch.empty(n_b + 1, dtype=torch.int64, device=device)
            col_out = torch.empty(max(nnz, 1), dtype=torch.int32,
                                  device=device)
            val_out = torch.empty(max(nnz, 1), dtype=torch.float64,
                                  device=device)
            counts = torch.zeros(2, dtype=torch.int64, device=device)
            _check(lib.remap_csr_from_coo(
                n_b, n_a, nnz, _ptr(row_d), _ptr(col_d), _ptr(s_d),
                int(index_base), _ptr(rowptr), _ptr(col_out), _ptr(val_out),
                ctypes.c_void_p(counts.data_ptr()),
                ctypes.c_void_p(counts.data_ptr() + 8), _ptr(ws),
                ws.numel(), _stream_ptr(device)), 'remap_csr_from_coo')
            nnz_u, bad = (int(v) for v in counts.cpu())
        if bad:
            raise ValueError(
                f'{bad} mapping triplets have a row or col index outside '
                f'the ({n_b}, {n_a}) matrix')
        return cls(n_a, n_b, rowptr, col_out[:nnz_u].clone(),
                   val_out[:nnz_u].clone(), frac_d)

    @classmethod
    def from_csr(cls, indptr, indices, data, frac_b, n_a, device=None):
        """
        Take an existing (host or device) CSR.  The kernels and the schedule
        builders rely on the canonical form scipy produces (``rowptr``
        monotone from 0 to ``len(indices)``, columns in range, ascending and
        unique within a row), so the input is validated and then rebuilt
        through the same device COO -> CSR path as a mapping file: unsorted
        rows are sorted and duplicate entries summed, as
        ``csr_matrix.sum_duplicates`` would.
        """
        torch = require_gpu()
        if device is None:
            device = torch.device('cuda', torch.cuda.current_device())
        rowptr = torch.as_tensor(indptr).to(device=device, dtype=torch.int64)
        n_b = int(rowptr.shape[0]) - 1
        col = torch.as_tensor(indices).to(device=device)
        val = torch.as_tensor(data).to(device=device, dtype=torch.float64)
        if n_b < 0 or col.shape[0] != val.shape[0]:
            raise ValueError('indptr must hold n_b + 1 entries and indices, '
                             'data the same number of entries')
        if n_b >= 0 and rowptr.numel():
            lens = rowptr[1:] - rowptr[:-1]
            if int(rowptr[0]) != 0 or int(rowptr[-1]) != col.shape[0] or \
                    (lens.numel() and int(lens.min()) < 0):
                raise ValueError(
                    'indptr must rise monotonically from 0 to len(indices)')
        else:
            lens = rowptr[:0]
        row = torch.repeat_interleave(
            torch.arange(n_b, device=device, dtype=torch.int32), lens)
        return cls.from_triplets(row, col, val, frac_b, n_a, n_b,
                                 index_base=0, device=device)

    # -- sharding -----------------------------------------------------------
    def shard_bounds(self, world_size):
        """
        Contiguous destination-row ranges, balanced by the work per row
        (entries + a constant per row for the output write), as a list of
        ``world_size + 1`` row indices.
        """
        from pyremap_amd.parallel import row_shard_bounds
        return row_shard_bounds(self.rowptr, world_size)

    def shard(self, rank, world_size):
        """The plan of rank ``rank`` of ``world_size`` (rows only)."""
        bounds = self.shard_bounds(world_size)
        return self.row_slice(bounds[rank], bounds[rank + 1])

    def row_slice(self, r0, r1):
        j0 = int(self.rowptr[r0])
        j1 = int(self.rowptr[r1])
        return RemapPlan(
            self.n_a, r1 - r0, (self.rowptr[r0:r1 + 1] - j0).contiguous(),
            self.col[j0:j1].contiguous(), self.val[j0:j1].contiguous(),
            self.frac_b[r0:r1].contiguous(),
            row_offset=self.row_offset + r0, n_b_global=self.n_b_global)

    def to(self, device):
        """A copy of this plan (CSR + frac_b, no schedule) on ``device``."""
        torch = _torch()
        device = torch.device(device)
        return RemapPlan(
            self.n_a, self.n_b, self.rowptr.to(device),
            self._col_padded.to(device), self._val_padded.to(device),
            self.frac_b.to(device), row_offset=self.row_offset,
            n_b_global=self.n_b_global)

    def packed(self):
        """
        This plan over the COMPACT space of the source rows it references
        (a row shard needs ``X[unique(col[shard])]``
        and nothing else): returns ``(plan, ucols)`` where ``ucols`` is the
        ascending int32 device tensor of the distinct source rows and
        ``plan`` is the same matrix with ``n_a = len(ucols)`` and every
        column index replaced by its position in ``ucols``
        (``remap_pack_columns``).  The renumbering is monotone, so a row's
        entries keep their order and the packed plan applied to
        ``X[ucols]`` gives the same bits as this plan applied to ``X``.
        Schedules are not carried over (they hold column indices): call
        ``auto_schedule`` on the result.
        """
        torch = _torch()
        lib = load_library()
        dev = self.device
        with torch.cuda.device(dev):
            nbytes = ctypes.c_size_t(0)
            _check(lib.remap_pack_columns_workspace(
                self.n_a, ctypes.byref(nbytes)),
                'remap_pack_columns_workspace')
            ws = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8,
                             device=dev)
            col = torch.zeros(self.nnz + CSR_PAD, dtype=torch.int32,
                              device=dev)
            ucols = torch.empty(max(min(self.nnz, self.n_a), 1),
                                dtype=torch.int32, device=dev)
            counts = torch.zeros(2, dtype=torch.int64, device=dev)
            _check(lib.remap_pack_columns(
                _ptr(self.col), self.nnz, self.n_a, _ptr(col), _ptr(ucols),
                ctypes.c_void_p(counts.data_ptr()),
                ctypes.c_void_p(counts.data_ptr() + 8), _ptr(ws),
                ws.numel(), _stream_ptr(dev)), 'remap_pack_columns')
            n_u, bad = (int(v) for v in counts.cpu())
        if bad:
            raise EngineError(f'{bad} column indices outside [0, {self.n_a})')
        plan = RemapPlan(n_u, self.n_b, self.rowptr, col, self._val_padded,
                         self.frac_b, row_offset=self.row_offset,
                         n_b_global=self.n_b_global)
        return plan, ucols[:n_u].clone()

    # -- scheduling ---------------------------------------------------------
    def set_row_order(self, order):
        """
        Install (or clear, with ``None``) the processing order of the rows:
        a permutation of ``range(n_b)``.  Results never depend on it.
        """
        torch = _torch()
        if order is None:
            self.row_order = None
            return
        order = torch.as_tensor(order).to(device=self.device,
                                          dtype=torch.int32).contiguous()
        if order.shape != (self.n_b,):
            raise ValueError(f'row order must have {self.n_b} entries')
        self.row_order = order

    def set_grid_schedule(self, grid_dims, kind='tile', tile=(32, 64)):
        """
        Walk a 2-D destination grid (``grid_dims`` = C-order dims of the
        WHOLE mapping's destination) in tiles or along a Morton curve, so
        rows that are neighbours in either direction -- and therefore share
        source rows -- are computed close together in time and on the same
        XCD.  1-D destinations keep their natural order.
        """
        torch = _torch()
        if grid_dims is None or len(grid_dims) != 2 or kind in (None, 'none'):
            self.row_order = None
            return
        my, mx = (int(d) for d in grid_dims)
        if my * mx != self.n_b_global:
            raise ValueError(f'grid {grid_dims} does not hold '
                             f'{self.n_b_global} cells')
        rows = torch.arange(self.row_offset, self.row_offset + self.n_b,
                            device=self.device, dtype=torch.int64)
        jy = rows // mx
        jx = rows - jy * mx
        if kind == 'tile':
            ty, tx = (int(t) for t in tile)
            ntx = (mx + tx - 1) // tx
            key = ((jy // ty) * ntx + jx // tx) * (ty * tx) + \
                (jy % ty) * tx + jx % tx
        elif kind == 'morton':
            key = torch.zeros_like(rows)
            for bit in range(16):
                key |= ((jx >> bit) & 1) << (2 * bit)
                key |= ((jy >> bit) & 1) << (2 * bit + 1)
        else:
            raise ValueError(f'unknown schedule {kind!r}')
        self.row_order = torch.argsort(key, stable=True).to(torch.int32)

    def _csr_struct(self):
        csr = _CSR()
        csr.n_rows, csr.n_cols, csr.nnz = self.n_b, self.n_a, self.nnz
        csr.rowptr = self.rowptr.data_ptr()
        csr.col = self.col.data_ptr()
        csr.val = self.val.data_ptr()
        csr.max_row_nnz, csr.csr_pad = self.max_row_nnz, self.csr_pad
        return csr

    def build_patches(self, grid_dims=None, tile=(4, 8), lds_budget=80 * 1024,
                      row_bytes=1024):
        """
        Build the LDS-staging schedule (``remap_apply_args.patch_*``) with
        the library's device builder (``remap_patches_build``): destination
        rows are walked in ``tile`` order over a 2-D grid (natural order for
        1-D destinations), ``tile[0] * tile[1]`` consecutive work slots form
        a patch, and for every patch the distinct source rows are listed
        once.  The tile is halved until the longest list fits the LDS budget
        (``row_bytes`` per staged source-row chunk).  Returns the fraction
        distinct / entries (small = much reuse), or ``None`` if no patch size
        fits.
        """
        def fits(rows, umax, emax):
            # entries staged next to the rows: 12 B each (+24 B per row)
            return (umax + 1) * row_bytes + emax * 12 + rows * 24 + 32 <= \
                lds_budget
        q = self._make_patches(grid_dims, tile, fits, row_bytes)
        if q is None:
            self.patches = None
            if self.nnz and self.n_b:
                self.row_order = None
            return None
        self.row_order = q['order']
        self.patches = q
        return q['distinct'] / self.nnz

    def _make_patches(self, grid_dims, tile, fits, row_bytes):
        """``remap_patches_build`` with ``tile``, halved until ``fits(rows,
        umax, emax)``; returns the plan's arrays as a dict, or ``None``."""
        torch = _torch()
        lib = load_library()
        if self.nnz == 0 or self.n_b == 0:
            return None
        dev = self.device
        ty, tx = (int(t) for t in tile)
        two_d = grid_dims is not None and len(grid_dims) == 2
        dims = None
        if two_d:
            my, mx = (int(d) for d in grid_dims)
            if my * mx != self.n_b_global:
                raise ValueError(f'grid {grid_dims} does not hold '
                                 f'{self.n_b_global} cells')
            dims = (ctypes.c_int64 * 2)(my, mx)
        csr = self._csr_struct()
        with torch.cuda.device(dev):
            nbytes = ctypes.c_size_t(0)
            _check(lib.remap_patches_workspace(self.n_b, self.nnz,
                                               ctypes.byref(nbytes)),
                   'remap_patches_workspace')
            ws = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8,
                             device=dev)
            ucol = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            prow = torch.empty(self.n_b + 1, dtype=torch.int32, device=dev)
            lidx = torch.empty(self.nnz, dtype=torch.int32, device=dev)
            pval = torch.empty(self.nnz, dtype=torch.float64, device=dev)
            order = torch.empty(self.n_b, dtype=torch.int32, device=dev) \
                if two_d else None
            stats = torch.zeros(3, dtype=torch.int64, device=dev)
            while True:
                rows = ty * tx
                n_patches = (self.n_b + rows - 1) // rows
                ptr = torch.empty(n_patches + 1, dtype=torch.int32,
                                  device=dev)
                _check(lib.remap_patches_build(
                    ctypes.byref(csr), dims, self.row_offset, ty, tx,
                    _ptr(order), _ptr(ptr), _ptr(ucol), _ptr(prow),
                    _ptr(lidx), _ptr(pval), _ptr(stats), _ptr(ws),
                    ws.numel(), _stream_ptr(dev)), 'remap_patches_build')
                distinct, umax, emax = (int(v) for v in stats.cpu())
                if fits(rows, umax, emax):
                    break
                if rows == 1:
                    return None
                if tx >= ty and tx > 1:
                    tx //= 2
                else:
                    ty //= 2
        return dict(
            ptr=ptr, ucol=ucol[:max(distinct, 1)].clone(), rowptr=prow,
            lidx=lidx, val=pval, rows=rows, umax=umax, emax=emax,
            n=n_patches, order=order, tile=(ty, tx), distinct=distinct,
            row_bytes=int(row_bytes))

    #: distinct source cells a patch of the lanes-across-rows kernel may
    #: stage: two cells per lane of a 1 024-thread workgroup, two LDS images
    #: of 4 fields each = 128 KB (spmm_patchtime)
    CELL_UMAX = 2046

    def run_patches(self):
        """
        Small LDS patches (4 x 8 tiles of the destination grid, 32
        consecutive rows of a 1-D one) for ``(Time, nCells, L)`` fields with
        SHORT level runs, 4 <= L < 16, on mappings whose own schedule is the
        row groups: there every (source row, batch) is a separate 32-120 byte
        run, the row-group kernel pays a line fetch per run and ENTRY, the
        LDS patch kernel (family 5) one per run and DISTINCT source row
        (config 3's map, fraction of 8 TB/s, groups / patches: L = 4 0.19 /
        0.27, 6 0.19 / 0.27, 8 0.39 / 0.45, 10 0.28 / 0.38, 12 0.34 / 0.41;
        from L = 16 the groups win, 0.60 / 0.55).  Built on first use;
        ``None`` when there is nothing to build.
        """
        if self._runs is None:
            dims = self._grid_dims
            if dims is not None and len(dims) != 2:
                dims = None

            def fits(rows, umax, emax):
                return (umax + 1) * 1024 + emax * 12 + rows * 24 + 32 <= \
                    100 * 1024 or rows <= 4
            q = self._make_patches(dims, (4, 8) if dims is not None
                                   else (1, 32), fits, 1024)
            self._runs = q if q is not None else False
            self._sched_version += 1
        return self._runs or None

    def run_cells(self):
        """
        The patch plan of the batch-at-a-time lanes-across-rows kernel
        (``spmm_patchtime<..., RUNS>``) for ``(Time, nCells, L)`` fields with
        VERY short level runs, 4 <= L <= ``RUN_CELLS_MAX``: 16 x 16 tiles (256
        consecutive rows of a 1-D destination), halved until a patch holds at
        most 510 source cells -- one 256-thread workgroup per patch walks the
        batches, the results of a batch leave through LDS as whole lines
        (config 3's map, ms per launch, this kernel / the small LDS patches
        of :meth:`run_patches` / row groups: L = 4 0.58 / 0.79 / 1.11, 5
        0.70 / 0.99 / 1.54, 6 0.74 / 0.77 / 1.12; from L = 8 the LDS patches
        win: 0.68 / 0.53 / 0.61).  Built on first use.
        """
        if self._run_cells is None:
            dims = self._grid_dims
            if dims is not None and len(dims) != 2:
                dims = None
            q = self._make_patches(
                dims, (16, 16) if dims is not None else (1, 256),
                lambda rows, umax, emax: umax <= 510 or rows <= 16, 1024)
            self._run_cells = q if q is not None else False
            self._sched_version += 1
        return self._run_cells or None

    #: longest level run the batch-at-a-time kernel takes (see run_cells)
    RUN_CELLS_MAX = 6

    def cell_patches(self):
        """
        The patch plan of kernel family 7 (``spmm_patchcell``), which serves
        fields whose contiguous run behind the source axes is short --
        (Time, nCells), the reference's most common input -- built on first
        use: 16 x 16 tiles of the destination grid (256 consecutive rows of a
        1-D destination), halved until no patch references more than
        ``CELL_UMAX`` distinct source cells.  ``None`` when there is nothing
        to build.
        """
        if self._cell is None:
            dims = self._grid_dims
            if dims is not None and len(dims) != 2:
                dims = None
            # (small grids: smaller tiles, so that there still are a few
            # hundred workgroups)
            tile = self.CELL_TILE
            while tile[0] * tile[1] > 256 and \
                    self.n_b < 128 * tile[0] * tile[1]:
                tile = (tile[0], tile[1] // 2) if tile[1] >= tile[0] else \
                    (tile[0] // 2, tile[1])
            def build(tile):
                return self._make_patches(
                    dims, tile if dims is not None
                    else (1, tile[0] * tile[1]),
                    lambda rows, umax, emax: umax <= self.CELL_UMAX or
                    rows <= 16, 1024)
            q = build(tile)
            # coarse -> fine (a patch stages fewer than half as many source
            # cells as it has rows): the output stores are the work, and
            # four 256-thread workgroups do them sooner than one of 1 024 --
            # 1 deg -> 0.5 deg bilinear, short rows, (12, n) 20.3 -> 17.3 us,
            # (120, n) float32 75.8 -> 71.9
            # (only where the large patches are few -- 254 there; config 4's
            # map, 29 K patches of 32 x 32, loses with the small ones: (32, n)
            # 3.3 -> 5.7 ms)
            if q is not None and q['rows'] > 256 and \
                    2 * q['umax'] < q['rows'] and q['n'] < 1024:
                ty, tx = q['tile']
                while ty * tx > 256:
                    ty, tx = (ty, tx // 2) if tx >= ty else (ty // 2, tx)
                q = build((ty, tx))
            self._cell = q if q is not None else False
            self._sched_version += 1
        return self._cell or None

    #: tile of the destination grid a patch of cell_patches covers (halved
    #: until a patch holds at most CELL_UMAX source cells): one 1 024-thread
    #: workgroup per patch and CU walks ALL its chunks -- config 3's map,
    #: (120, nCells) cold: 16 x 16 / 16 x 32 / 32 x 32 tiles 0.146 / 0.137 /
    #: 0.121 ms
    CELL_TILE = (32, 32)

    GROUP = 8   # default rows per group (remap_apply_args.group_rows)

    def build_groups(self, grid_dims=None, super_tile=32, rows=None,
                     share=0):
        """
        Build the row-group schedule (``remap_apply_args.group_*``) with the
        library's device builder (``remap_groups_build``): ``rows`` (8 or 4)
        consecutive work slots -- a 2 x 4 or 2 x 2 tile of a 2-D destination
        grid, walked row-major inside ``super_tile`` x ``super_tile`` blocks
        -- share one sorted list of the distinct source rows they reference;
        the weights are stored for the present (union entry, member) pairs
        only, in that order.  Returns union entries / entries (small = many
        shared source rows).

        ``share`` = 2 or 4: also build the SHARED union lists of the shared
        form (``csrc/spmm_sharering.h``, ``remap_share_build``): 2 / 4
        consecutive 8-row groups -- a 4 x 4 / 4 x 8 tile of the grid, walked
        row-major inside the supertiles -- get one union served by one
        workgroup through LDS.  ``groups['share']['ratio']`` is their union
        entries / entries.
        """
        torch = _torch()
        lib = load_library()
        G = int(rows or self.GROUP)
        if G not in (4, 8, 16):
            raise ValueError('row groups hold 4, 8 or 16 rows')
        share = int(share or 0)
        if share:
            if share not in (2, 4) or G != 8:
                raise ValueError('shared lists: 2 or 4 groups of 8 rows')
            if int(super_tile) < (1 << 30) and int(super_tile) % (2 * share):
                raise ValueError('super_tile must hold whole 4 x '
                                 f'{2 * share} supergroup tiles')
        self.groups = None
        if self.nnz == 0 or self.n_b == 0:
            return None
        dev = self.device
        two_d = grid_dims is not None and len(grid_dims) == 2
        dims = None
        if two_d:
            my, mx = (int(d) for d in grid_dims)
            if my * mx != self.n_b_global:
                raise ValueError(f'grid {grid_dims} does not hold '
                                 f'{self.n_b_global} cells')
            dims = (ctypes.c_int64 * 2)(my, mx)
        st = int(super_tile)
        if st >= 1 << 30:
            st = 0           # no supertiles: row-major over the whole grid
        n_groups = (self.n_b + G - 1) // G
        meta = torch.empty((n_groups + 1, 2), dtype=torch.int64, device=dev)
        col = torch.empty(self.nnz + 32, dtype=torch.int32, device=dev)
        mask = torch.empty(self.nnz + 32, dtype=torch.int32, device=dev)
        w = torch.empty(self.nnz + 128, dtype=torch.float64, device=dev)
        rid = torch.empty(n_groups * G, dtype=torch.int32, device=dev)
        frac = torch.empty(n_groups * G, dtype=torch.float64, device=dev)
        order = torch.empty(self.n_b, dtype=torch.int32, device=dev) \
            if two_d else None
        n_union = torch.zeros(1, dtype=torch.int64, device=dev)
        csr = self._csr_struct()
        with torch.cuda.device(dev):
            nbytes = ctypes.c_size_t(0)
            _check(lib.remap_groups_workspace(self.n_b, self.nnz,
                                              ctypes.byref(nbytes)),
                   'remap_groups_workspace')
            ws = torch.empty(max(int(nbytes.value), 1), dtype=torch.uint8,
                             device=dev)
            _check(lib.remap_groups_build(
                ctypes.byref(csr), _ptr(self.frac_b), G, dims,
                self.row_offset, st, share, _ptr(order), _ptr(meta),
                _ptr(col),
                _ptr(mask), _ptr(w), _ptr(rid), _ptr(frac), _ptr(n_union),
                _ptr(ws), ws.numel(), _stream_ptr(dev)),
                'remap_groups_build')
            nu = int(n_union)
        self.row_order = order
        # trim the union arrays to what is used (+ the readable pad)
        groups = dict(meta=meta, col=col[:nu + 32].clone(),
                      w=w, mask=mask[:nu + 32].clone(), rid=rid,
                      frac=frac, n=n_groups, rows=G, order=order,
                      union=nu)
        if share:
            n_super = (self.n_b + 8 * share - 1) // (8 * share)
            smeta = torch.empty((n_super + 1, 2), dtype=torch.int64,
                                device=dev)
            # (col / mask above are free again: trimmed copies were taken)
            scol = torch.empty(self.nnz + 256, dtype=torch.int32, device=dev)
            smask = torch.empty(self.nnz + 256, dtype=torch.int32,
                                device=dev)
            with torch.cuda.device(dev):
                _check(lib.remap_share_build(
                    ctypes.byref(csr), _ptr(rid), share, _ptr(smeta),
                    _ptr(scol), _ptr(smask), _ptr(n_union), _ptr(ws),
                    ws.numel(), _stream_ptr(dev)), 'remap_share_build')
                su = int(n_union)
            groups['share'] = dict(meta=smeta, col=scol[:su + 256].clone(),
                                   mask=smask[:su + 256].clone(),
                                   waves=share, union=su,
                                   ratio=su / self.nnz)
        self.groups = groups
        return nu / self.nnz

    #: a row counts as LONG from this many entries on (the widest stencils
    #: of ordinary maps -- 2nd-order conservative -- hold ~30)
    LONG_ROW = 96

    def build_strips(self, grid_dims, **shape):
        """
        Attach the strip schedule of kernel family 8 (``csrc/spmm_strip.h``):
        an LDS ring of source-row pieces sliding along strips of the
        destination grid ``grid_dims``, for entry-rich mappings (2nd-order
        conservative stencils).  ``shape``: ``strip_rows``, ``step_cols``,
        ``segments``, ``depth`` (:func:`pyremap_amd.strips.build_strips`).
        Calls the kernel cannot serve (several batches, float32, a row
        shard) run on the plan's other schedule as before.  Raises
        :class:`pyremap_amd.strips.StripsUnfit` when the ring does not fit
        the LDS.
        """
        from pyremap_amd import strips as _strips
        if self.row_offset != 0 or self.n_b != self.n_b_global:
            raise ValueError('a strip schedule covers a whole mapping')
        st = _strips.build_strips(self, grid_dims, **shape)
        st['struct'] = _strips.struct(st, _Strips)
        self.strips = st
        return st

    def _split_long_rows(self):
        """
        Mappings whose few LONG rows hold a large share of the entries -- a
        global lat-lon bilinear map as ESMF makes it: the destination cells
        poleward of the last source row take the WHOLE adjacent source row
        (the pole cap, ``weights.bilinear_3d``), 362-1 442 entries per row
        among rows of 4, a third of all entries in 0.6 % of the rows -- lose
        every schedule built for short rows (no LDS patch holds 1 440 source
        rows) and serialise the others (a lane walks its row entry by entry:
        1 deg -> 0.5 deg, one 2-D field, 66 us against 13 us without the caps;
        K = 64: 150 against 37).

        Such a plan is applied as TWO launches writing disjoint rows: the
        mapping without the long rows' entries on its own schedule, and the
        long rows through the LDS-staged lanes-across-rows kernel (family 7):
        the source rows they share are staged once per 256 rows, every lane
        sums its row in CSR order from LDS.  Returns ``(short, long)`` plans
        or ``None`` when the mapping has no such rows (or the long rows'
        sources do not fit the LDS).
        """
        torch = _torch()
        if self.max_row_nnz <= self.LONG_ROW:
            return None
        counts = self.rowptr[1:] - self.rowptr[:-1]
        is_long = counts > self.LONG_ROW
        ids = is_long.nonzero().squeeze(1)
        n_long = int(ids.shape[0])
        long_entries = int(counts[ids].sum())
        if n_long == 0 or n_long > self.n_b // 8 or \
                long_entries < self.nnz // 50:
            return None
        entry_long = torch.repeat_interleave(is_long, counts)

        def sub(rows_kept, entries_kept, n_rows, **where):
            rp = torch.zeros(n_rows + 1, dtype=torch.int64,
                             device=self.device)
            rp[1:] = torch.cumsum(rows_kept, 0)
            return RemapPlan(self.n_a, n_rows, rp,
                             self.col[entries_kept].contiguous(),
                             self.val[entries_kept].contiguous(),
                             self.frac_b, **where)
        # (a row shard splits like a whole mapping: same place in the grid)
        short = sub(torch.where(is_long, torch.zeros_like(counts), counts),
                    ~entry_long, self.n_b, row_offset=self.row_offset,
                    n_b_global=self.n_b_global)
        long = sub(counts[ids], entry_long, n_long)
        # the long rows' patch plan: 256 consecutive long rows per workgroup,
        # halved until the distinct source rows fit the LDS with 4 fields
        # per lane; work slot -> row of the WHOLE mapping
        limit = CELL_LDS_MAX // (4 * 8) - 2
        q = long._make_patches(None, (1, 256),
                               lambda rows, umax, emax: umax <= limit, 1024)
        if q is None:
            return None
        q['order'] = ids.to(torch.int32).contiguous()
        # many fields: a wave per long row, the source cells of a few
        # neighbouring rows sliding through LDS (family 11) -- row-major
        # entries whose local indices do not decrease inside a row (they
        # cannot: the rows are sorted by column; checked all the same)
        long._wave = None
        # (its LDS image per row: two windows of 8 cells x 512 bytes and the
        # row's records, 12 bytes each -- run_longwave)
        per_row = 2 * 8 * 512 + ((long.max_row_nnz + 15) // 16 * 16 + 16) * 12
        wave_rows = min(int(LONG_WAVE_ROWS), CELL_LDS_MAX // per_row)
        if wave_rows >= 1:
            w = long._make_patches(None, (1, wave_rows),
                                   lambda rows, umax, emax: True, 1024)
            if w is not None:
                li = w['lidx'][:long.nnz]
                first = torch.zeros(long.nnz, dtype=torch.bool,
                                    device=self.device)
                first[w['rowptr'][:-1].to(torch.int64)
                      .clamp_(max=long.nnz - 1)] = True
                if bool(((li[1:] >= li[:-1]) | first[1:]).all()):
                    w['order'] = q['order']
                    long._wave = w
        rows, n_p = q['rows'], q['n']
        rp = q['rowptr'].to(torch.int64)
        lens = rp[1:] - rp[:-1]
        slot = torch.arange(n_long, device=self.device)
        patch, r_local = slot // rows, slot % rows
        e_slot = torch.repeat_interleave(slot, lens)
        j = torch.arange(long.nnz, device=self.device) - rp[e_slot]
        lidx, val = q['lidx'][:long.nnz], q['val'][:long.nnz]
        # the entries COLUMN-MAJOR inside every patch (patch_ell_base):
        # the lanes -- one slot each -- read their j-th entries with one
        # coalesced load instead of a line fetch per lane and entry
        longest = torch.zeros(n_p, dtype=torch.int64,
                              device=self.device) \
            .scatter_reduce(0, patch, lens, 'amax')
        base = torch.cumsum(longest * rows, 0) - longest * rows
        dest = base[patch[e_slot]] + j * rows + r_local[e_slot]
        total = int((longest * rows).sum())
        val_t = torch.zeros(total + CSR_PAD, dtype=torch.float64,
                            device=self.device)
        lidx_t = torch.zeros(total + CSR_PAD, dtype=torch.int32,
                             device=self.device)
        val_t[dest] = val
        lidx_t[dest] = lidx
        q['val'], q['lidx'] = val_t, lidx_t
        q['ell_base'] = base.contiguous()
        q['layout'] = 'column-major'
        long._cell = q
        return short, long

    def auto_schedule(self, grid_dims, _split_ok=True):
        """
        Choose AND build the schedule for this mapping with the library's
        ``remap_schedule_auto`` (the rules -- LDS patches for heavily shared,
        short rows; row groups where rows share columns at all; the plain
        kernel otherwise -- live there, next to the measurements they come
        from: ``csrc/remap_schedule.hip``).  The
        schedule's arrays are views into one device arena owned by the plan.
        Returns the description of what was chosen.
        """
        torch = _torch()
        lib = load_library()
        self.patches = None
        self.groups = None
        self.row_order = None
        self.default_tune = None
        self._arena = None
        self._cell = None
        self._runs = None
        self._run_cells = None
        self._grid_dims = None
        self._split = None
        if grid_dims is None or self.nnz == 0 or self.n_b == 0:
            return {'family': 'rowscalar', 'reason': 'no destination grid'}
        if _split_ok:
            split = self._split_long_rows()
            if split is not None:
                short, long = split
                choice = short.auto_schedule(grid_dims, _split_ok=False)
                self._split = split
                self._grid_dims = short._grid_dims
                return dict(choice, long_rows=long.n_b,
                            long_row_entries=long.nnz,
                            long_rows_layout=long._cell['layout'])
        dims = tuple(int(d) for d in grid_dims)
        if len(dims) in (1, 2) and _prod(dims) == self.n_b_global:
            self._grid_dims = dims
        if len(dims) not in (1, 2):
            return {'family': 'rowscalar',
                    'reason': f'{len(dims)}-D destination grid'}
        if _prod(dims) != self.n_b_global:
            raise ValueError(f'grid {dims} does not hold '
                             f'{self.n_b_global} cells')
        dev = self.device
        sched = _Schedule()
        csr = self._csr_struct()
        cdims = (ctypes.c_int64 * len(dims))(*dims)
        with torch.cuda.device(dev):
            a_bytes, w_bytes = ctypes.c_size_t(0), ctypes.c_size_t(0)
            _check(lib.remap_schedule_sizes(
                self.n_b, self.nnz, ctypes.byref(a_bytes),
                ctypes.byref(w_bytes)), 'remap_schedule_sizes')
            arena = torch.empty(int(a_bytes.value), dtype=torch.uint8,
                                device=dev)
            ws = torch.empty(max(int(w_bytes.value), 1), dtype=torch.uint8,
                             device=dev)
            _check(lib.remap_schedule_auto(
                ctypes.byref(csr), _ptr(self.frac_b), cdims, len(dims),
                self.row_offset, _ptr(arena), arena.numel(), _ptr(ws),
                ws.numel(), ctypes.byref(sched), _stream_ptr(dev)),
                'remap_schedule_auto')
            del ws
            if sched.family in (5, 10) and \
                    sched.arena_used < arena.numel() // 2:
                # keep only what the schedule occupies (the arena was sized
                # for the larger of the two candidate layouts)
                used = (int(sched.arena_used) + 255) // 256 * 256
                small = arena[:used].clone()
                shift = small.data_ptr() - arena.data_ptr()
                for name, ctype in _Schedule._fields_:
                    v = getattr(sched, name)
                    if ctype is ctypes.c_void_p and v and \
                            arena.data_ptr() <= v < arena.data_ptr() + used:
                        setattr(sched, name, v + shift)
                arena = small
        base = arena.data_ptr()

        def view(ptr, count, dtype):
            if not ptr:
                return None
            nbytes = count * torch.empty((), dtype=dtype).element_size()
            return arena[ptr - base:ptr - base + nbytes].view(dtype)

        self._arena = arena
        order = view(sched.row_order, self.n_b, torch.int32)
        tune = {mode: [int(v) for v in sched.tune[mode]][:6]
                for mode in (MODE_RAW, MODE_FRACB, MODE_MASKED)}
        if sched.family == 5:
            self.row_order = order
            n_p = int(sched.n_patches)
            self.patches = dict(
                ptr=view(sched.patch_ptr, n_p + 1, torch.int32),
                ucol=view(sched.patch_ucol, max(int(sched.n_distinct), 1),
                          torch.int32),
                rowptr=view(sched.patch_rowptr, self.n_b + 1, torch.int32),
                lidx=view(sched.patch_lidx, self.nnz, torch.int32),
                val=view(sched.patch_val, self.nnz, torch.float64),
                rows=int(sched.patch_rows), umax=int(sched.patch_umax),
                emax=int(sched.patch_emax), n=n_p, order=order,
                tile=(int(sched.tile_y), int(sched.tile_x)),
                distinct=int(sched.n_distinct),
                row_bytes=int(sched.patch_row_bytes))
            return {'family': 'patch', 'tile': self.patches['tile'],
                    'ratio': float(sched.ratio),
                    'umax': self.patches['umax'],
                    'row_bytes': self.patches['row_bytes']}
        if sched.family == 10:
            self.row_order = order
            n_g, G = int(sched.n_groups), int(sched.group_rows)
            nu = int(sched.n_distinct)
            self.groups = dict(
                meta=view(sched.group_meta, 2 * (n_g + 1),
                          torch.int64).reshape(n_g + 1, 2),
                col=view(sched.group_col, nu + 32, torch.int32),
                w=view(sched.group_w, self.nnz + 128, torch.float64),
                mask=view(sched.group_mask, nu + 32, torch.int32),
                rid=view(sched.group_rid, n_g * G, torch.int32),
                frac=view(sched.group_frac, n_g * G, torch.float64),
                n=n_g, rows=G, order=order, union=nu)
            share = None
            if sched.share_waves:
                W, su = int(sched.share_waves), int(sched.n_share_union)
                n_s = (self.n_b + 8 * W - 1) // (8 * W)
                share = dict(
                    meta=view(sched.share_meta, 2 * (n_s + 1),
                              torch.int64).reshape(n_s + 1, 2),
                    col=view(sched.share_col, su + 256, torch.int32),
                    mask=view(sched.share_mask, su + 256, torch.int32),
                    waves=W, union=su, ratio=su / self.nnz)
                self.groups['share'] = share
                # (assigning into the dict does not pass the property)
                self._sched_version += 1
            self.default_tune = tune
            rich = bool(sched.entry_rich)
            out = {'family': 'rowgroup', 'union_ratio': float(sched.ratio),
                   'rows_per_group': G,
                   'order': '2x4 groups in 32x32 supertiles' if rich
                   else '2x2 groups, row-major' if len(dims) == 2 else
                   '4 consecutive rows', 'tune': self.default_tune}
            if share is not None:
                out['shared_by'] = share['waves']
                out['shared_union_ratio'] = share['ratio']
                out['order'] = '2x4 groups in 4x8 tiles in 32x32 supertiles'
            return out
        if sched.family == 6:
            self.row_order = order.clone()
            self._arena = None
            self.default_tune = tune[MODE_FRACB]
            return {'family': 'rowscalar', 'order': 'tile 32x32',
                    'tune': self.default_tune,
                    'reason': 'entry-rich rows: keep the stencil band in L2'}
        self._arena = None
        return {'family': 'rowscalar', 'reason': 'little source-row reuse'}

    # -- accounting ---------------------------------------------------------
    def block_source_extent(self, rows_per_block):
        """
        For consecutive blocks of ``rows_per_block`` destination rows: one
        past the LAST source row any of the block's entries references, as a
        running maximum over the blocks (a list, one value per block).  A
        block can be computed once that many source rows are resident.
        Cached: the per-row maxima once per plan, the block values per size.
        """
        torch = _torch()
        rows_per_block = int(rows_per_block)
        if rows_per_block in self._extent_cache:
            return self._extent_cache[rows_per_block]
        if self._row_last_col is None:
            last = torch.zeros(self.n_b, dtype=torch.int64,
                               device=self.device)
            if self.nnz:
                # columns ascend within a row: the last entry is the largest
                lens = self.rowptr[1:] - self.rowptr[:-1]
                has = lens > 0
                last[has] = self.col[(self.rowptr[1:][has] - 1)].to(
                    torch.int64) + 1
            self._row_last_col = last
        n_blocks = (self.n_b + rows_per_block - 1) // rows_per_block
        padded = torch.zeros(n_blocks * rows_per_block, dtype=torch.int64,
                             device=self.device)
        padded[:self.n_b] = self._row_last_col
        hi = padded.reshape(n_blocks, rows_per_block).amax(dim=1)
        out = torch.cummax(hi, 0).values.cpu().tolist()
        self._extent_cache[rows_per_block] = out
        return out

    def touched_sources(self):
        """Number of DISTINCT source cells this plan's rows reference."""
        if self._touched is None:
            torch = _torch()
            hit = torch.zeros(self.n_a, dtype=torch.bool, device=self.device)
            if self.nnz:
                hit[self.col.to(torch.int64)] = True
            self._touched = int(hit.sum())
        return self._touched

    def algorithmic_bytes(self, K, x_itemsize=8, mode=MODE_FRACB):
        """
        SURVEY.md section 8(d): S + col read once, rowptr, X read once,
        Y written once, frac_b in the unmasked mode.  Only source rows that
        some entry references count towards X (a whole mapping touches every
        source cell, so this is ``n_a`` there; a row shard or a map with
        unreferenced cells moves fewer bytes and is priced accordingly).
        """
        b = self.nnz * 12 + (self.n_b + 1) * 8
        b += self.touched_sources() * K * x_itemsize + self.n_b * K * 8
        if mode == MODE_FRACB:
            b += self.n_b * 8
        return b

    def to_host_csr(self):
        return (self.rowptr.cpu().numpy(), self.col.cpu().numpy(),
                self.val.cpu().numpy())

    def transposed(self):
        """
        The plan of ``S^T``, ``(n_a, n_b)``, built on the device once and kept
        (:meth:`release_transposed` drops it): the triplets of this plan's CSR
        with row and column swapped through the COO -> CSR sort a mapping file
        takes, so inside a source cell the entries are in ascending destination
        row (:func:`pyremap_amd.adjoint.transpose` is the same statement in
        numpy).  Its ``frac_b`` is ones: it is applied in ``MODE_RAW``
        (:func:`remap_tensor_adjoint`).  Rows that hold a large share of the
        entries -- the source cells of a coarse -> fine map -- are kept apart
        as in any plan (:meth:`_split_long_rows`); no destination grid is
        known for it, so no other schedule is attached.  The build allocates
        and reads counts back: make it before capturing launches in a
        hipGraph.
        """
        hit = self.__dict__.get('_transposed')
        if hit is not None:
            return hit
        torch = _torch()
        _one_device(self, 'the transposed plan')
        if self.n_b != self.n_b_global:
            raise NotImplementedError(
                'the transposed plan of a row shard holds part of every sum: '
                'not with a sharded plan')
        _holds_csr(self, ('rowptr', 'col', 'val'),
                   'the transposed plan is sorted from its triplets')
        with torch.cuda.device(self.device):
            row = torch.repeat_interleave(
                torch.arange(self.n_b, dtype=torch.int32, device=self.device),
                self.rowptr[1:] - self.rowptr[:-1], output_size=self.nnz)
            t = RemapPlan.from_triplets(
                row=self.col, col=row, S=self.val,
                frac_b=torch.ones(self.n_a, dtype=torch.float64,
                                  device=self.device),
                n_a=self.n_b, n_b=self.n_a, index_base=0, device=self.device)
            t._split = t._split_long_rows()
        self._transposed = t
        return t

    def release_transposed(self):
        """Drop the plan :meth:`transposed` keeps (its device memory)."""
        self._transposed = None


# ---------------------------------------------------------------------------
# launches
# ---------------------------------------------------------------------------

def _float_dtype(torch, name, t):
    if t.dtype == torch.float64:
        return DTYPE_F64
    if t.dtype == torch.float32:
        return DTYPE_F32
    raise TypeError(f'{name} must be float64 or float32, not {t.dtype}')


def _one_device(plan, what):
    if hasattr(plan, 'shards') or not isinstance(plan, RemapPlan):
        raise NotImplementedError(
            f'{what} serves one device: not with a multi-device or '
            f'process-group plan')


def _holds_csr(plan, arrays, why):
    """The passes beside the apply read the plan's own CSR, never a schedule
    (a split plan keeps the whole mapping's CSR beside its two parts)."""
    sizes = {'rowptr': plan.n_b + 1, 'col': plan.nnz, 'val': plan.nnz}
    for name in arrays:
        t = getattr(plan, name)
        if t is None or t.numel() != sizes[name]:
            raise EngineError(f'the plan no longer holds its CSR '
                              f'({", ".join(arrays)}): {why}')


def _check_fold(n_a, x_src_fold, *outer_strides):
    if x_src_fold < 0 or n_a % x_src_fold or min(outer_strides) < 0:
        raise ValueError(f'x_src_fold {x_src_fold} does not divide '
                         f'n_a = {n_a}')


def _check_reach(name, t, rows, row_stride, batch_stride, inner_stride,
                 n_batch, k_inner, fold=0, outer_stride=0):
    """The kernels address through raw pointers: ``t`` must hold the last
    element the strides reach.  ``fold``: two source axes, the last cell is
    ``(rows / fold - 1, fold - 1)``."""
    if t is None or n_batch <= 0 or k_inner <= 0 or rows <= 0:
        return
    last = (rows - 1) * row_stride
    if fold:
        _check_fold(rows, fold, outer_stride)
        last = (rows // fold - 1) * outer_stride + (fold - 1) * row_stride
    reach = (n_batch - 1) * batch_stride + last + \
        (k_inner - 1) * inner_stride + 1
    if min(row_stride, batch_stride) < 0 or reach > t.numel():
        raise ValueError(
            f'{name} holds {t.numel()} elements; the strides (row '
            f'{row_stride}, batch {batch_stride}) reach {reach}')


def _row_range(plan, row_begin, row_end):
    end = plan.n_b if row_end is None else int(row_end)
    row_begin = int(row_begin)
    if not 0 <= row_begin <= end <= plan.n_b:
        raise ValueError(f'rows [{row_begin}, {end}) are not inside '
                         f'[0, {plan.n_b}]')
    return row_begin, end


def _launch(torch, plan, fn, name, args, enter=True):
    """``fn(args, stream)`` on torch's current stream of the plan's device;
    ``enter``: inside that device's context."""
    stream = ctypes.c_void_p(
        torch.cuda.current_stream(plan.device).cuda_stream)
    if enter:
        with torch.cuda.device(plan.device):
            _check(fn(ctypes.byref(args), stream), name)
    else:
        _check(fn(ctypes.byref(args), stream), name)


def apply_strided(plan, X, Y, *, n_batch, k_inner, x_row_stride,
                  x_batch_stride, y_row_stride, y_batch_stride, mode,
                  threshold=0.0, mask_out=None, flags=0, tune=None,
                  row_begin=0, row_end=None, gate=None, gate_value=0,
                  x_src_fold=0, x_outer_stride=0, _long_rows=False):
    """
    One asynchronous ``remap_apply_f64`` launch on torch's current stream.
    ``X``/``Y``/``mask_out`` are device tensors; strides are in elements.

    The first ``(Time, nCells)``-like call on a plan (short contiguous runs
    in several batches) builds the patch plan of ``spmm_patchcell``
    (:meth:`RemapPlan.cell_patches`: allocations and one readback): make it
    -- or call ``plan.cell_patches()`` -- before capturing launches in a
    hipGraph.

    ``mode=MODE_LAF`` (largest area fraction, :mod:`pyremap_amd.laf`) is a
    row pass over the plan's own CSR: ``flags``, ``tune`` and every schedule
    are ignored, nothing is built, one device only.  ``MODE_MIN``,
    ``MODE_MAX``, ``MODE_VAR`` and ``MODE_MEDIAN`` (sub-grid statistics,
    :mod:`pyremap_amd.rowstat`) are such passes too, and so is
    ``MODE_CLASSFRAC`` (:mod:`pyremap_amd.classfrac`), which reads its
    arguments in its own way: ``X`` is ONE batch of class indices
    (``x_batch_stride=0``), ``n_batch`` the number of classes and the batches
    of ``Y`` and ``mask_out`` are the classes
    (:func:`remap_tensor_fractions` is the entry that lays them out).
    """
    torch = _torch()
    lib = load_library()
    if mode in (MODE_COTAN_FRACB, MODE_COTAN_MASKED):
        raise ValueError('the cotangent modes read their arguments in their '
                         'own way: cotangent_strided launches them')
    if mode in _ROW_PASS_MODES:
        _one_device(plan, _ROW_PASS_MODES[mode])
    if X.device != plan.device or Y.device != plan.device:
        raise ValueError('X, Y and the plan must live on the same device')
    if Y.dtype != torch.float64:
        raise TypeError('Y must be float64')
    x_dtype = _float_dtype(torch, 'X', X)
    _check_reach('X', X, plan.n_a, x_row_stride, x_batch_stride, 1, n_batch,
                 k_inner, x_src_fold, x_outer_stride)
    for name, t in (('Y', Y), ('mask_out', mask_out)):
        _check_reach(name, t, plan.n_b, y_row_stride, y_batch_stride, 1,
                     n_batch, k_inner)
    if mask_out is not None and (mask_out.dtype != torch.uint8 or
                                 mask_out.device != plan.device):
        raise TypeError('mask_out must be a uint8 tensor on the plan device')
    end = plan.n_b if row_end is None else row_end
    if mode in _ROW_PASS_MODES:
        # a row pass over the plan's own CSR (csrc/apply_laf.h,
        # csrc/apply_rowstat.h, csrc/apply_classfrac.h): no schedule, no tune,
        # no split into short and long rows; flags mean nothing
        row_begin, end = _row_range(plan, row_begin, row_end)
        _holds_csr(plan, ('rowptr', 'col', 'val'),
                   f"{_ROW_PASS_MODES[mode]} adds a row's weights from it")
        args = _ApplyArgs()
        args.A = plan._csr_struct()
        args.row_begin, args.row_end = row_begin, end
        args.X, args.x_dtype, args.mode = X.data_ptr(), x_dtype, mode
        args.x_row_stride = int(x_row_stride)
        args.x_batch_stride = int(x_batch_stride)
        args.Y = Y.data_ptr()
        args.y_row_stride = int(y_row_stride)
        args.y_batch_stride = int(y_batch_stride)
        args.n_batch, args.k_inner = int(n_batch), int(k_inner)
        args.threshold = float(threshold)
        args.mask_out = mask_out.data_ptr() if mask_out is not None else None
        if gate is not None:
            if gate.dtype != torch.int32 or gate.device != plan.device:
                raise TypeError('gate must be an int32 tensor on the plan '
                                'device')
            args.gate = gate.data_ptr()
            args.gate_value = int(gate_value)
        args.x_src_fold = int(x_src_fold)
        args.x_outer_stride = int(x_outer_stride)
        _launch(torch, plan, lib.remap_apply_f64, 'remap_apply_f64', args)
        return
    whole = row_begin == 0 and end == plan.n_b
    if plan._split is not None and whole and not tune:
        # a few long rows hold a large share of the entries (pole caps of a
        # global bilinear map): two launches writing disjoint rows
        # (RemapPlan._split_long_rows)
        kw = dict(n_batch=n_batch, k_inner=k_inner,
                  x_row_stride=x_row_stride, x_batch_stride=x_batch_stride,
                  y_row_stride=y_row_stride, y_batch_stride=y_batch_stride,
                  mode=mode, threshold=threshold, mask_out=mask_out,
                  flags=flags, gate=gate, gate_value=gate_value,
                  x_src_fold=x_src_fold, x_outer_stride=x_outer_stride)
        short, long = plan._split
        # (Issuing the two launches on two streams joined by events -- they
        # write disjoint rows -- was built and measured: replayed from a
        # hipGraph the two branches still ran one after the other, K = 64
        # 63.5 us against 60.2; issued from Python the four extra stream
        # calls cost more than the overlap gave, 84 us against 61.  One
        # stream it stays.)
        for part, is_long in ((short, False), (long, True)):
            if part is None:      # (tools/long_rows_probe.py: one part alone)
                continue
            apply_strided(part, X, Y, _long_rows=is_long, **kw)
        return
    # short contiguous runs in several batches -- (Time, nCells) -- go to the
    # LDS-staged lanes-across-rows kernel on its own patch plan
    cell = _long_rows or (
        whole and not tune and
        ((k_inner < CELL_MAX_RUN and n_batch > 1) or x_src_fold) and
        n_batch * k_inner >= 2 and plan.cell_patches() is not None)
    # short level runs in several batches -- (Time, nCells, 4 ... 15) -- on
    # a row-group mapping: small LDS patches (RemapPlan.run_patches)
    if not cell and whole and not tune and n_batch > 1 and \
            4 <= k_inner < 16 and n_batch * k_inner >= 64 and \
            plan.patches is None:
        if k_inner <= plan.RUN_CELLS_MAX and plan.run_cells() is not None:
            cell = 'run_cells'
        elif plan.run_patches() is not None:
            cell = 'runs'
    if _long_rows and LONG_WAVE_FIELDS < n_batch * k_inner <= \
            LONG_WAVE_MAX and plan._wave is not None and LONG_WAVE_ROWS:
        cell = 'wave'
    args = plan._prefilled(whole, cell)
    if cell == 'wave':
        # many fields on long rows: one wave per row, the cells a few rows
        # share sliding through LDS (family 11, spmm_longwave.h)
        tune = [11]
        flags |= FLAG_TUNE_HINT
    elif cell == 'runs':
        tune = [5]
        flags |= FLAG_TUNE_HINT
    elif cell == 'run_cells':
        # 4 columns per chunk of the batch-at-a-time kernel; with 5 or 6
        # levels 6: the batch is ONE chunk (config 3's map, (80, n, 6):
        # 0.57 -> 0.47 ms, (96, n, 5): 0.70 -> 0.67)
        tune = list(_RUNS_TUNE) if _RUNS_TUNE else \
            [7, 6 if k_inner >= 5 else 4, 2]
        flags |= FLAG_TUNE_HINT
    elif cell:
        # 4 fields per lane and LDS image: the workgroup stays on its patch
        # over a run of chunks (spmm_patchtime), two images in LDS -- config
        # 3's map, Infinity-Cache-cold, 4 / 8 fields: (120, nCells) 0.141 /
        # 0.146 ms, (12, nCells) 16.4 / 24 us; (60, 3.7 M cells) 1.13 / 1.20
        tune = [7, 4]
        if _CELL_TUNE:
            tune = [7] + list(_CELL_TUNE)
        if _long_rows:
            K = n_batch * k_inner
            if K <= LONG_WAVE_FIELDS:
                # few fields: one wave per (long row, a few columns) -- the
                # row's loads run lanes-across-entries, only its sum is a
                # chain (family 9, spmm_longrow.h).  1 deg -> 0.5 deg with
                # pole caps, the long rows' launch: K = 1 15 -> 3 us
                tune = [9, _LONG_WAVE_TT or 0]
            else:
                # many fields: the 256 rows of a patch share their source
                # cells, staged once (family 7); a long row is ONE dependent
                # chain: few fields per lane keep its steps short and the
                # workgroups many (us per apply with 1 / 2 / 4 fields per
                # lane: K = 64 72 / 65 / 83, K = 512 423 / 352 / 320)
                tune = [7, _LONG_TT or (2 if K <= 128 else 4)]
        flags |= FLAG_TUNE_HINT
    args.row_begin = row_begin
    args.row_end = end
    args.X = X.data_ptr()
    args.x_dtype = x_dtype
    args.mode = mode
    args.x_row_stride = x_row_stride
    args.x_batch_stride = x_batch_stride
    args.Y = Y.data_ptr()
    args.y_row_stride = y_row_stride
    args.y_batch_stride = y_batch_stride
    args.n_batch = n_batch
    args.k_inner = k_inner
    args.frac_b = plan.frac_b.data_ptr() if mode == MODE_FRACB else None
    args.threshold = float(threshold)
    args.mask_out = mask_out.data_ptr() if mask_out is not None else None
    if gate is not None:
        if gate.dtype != torch.int32 or gate.device != plan.device:
            raise TypeError('gate must be an int32 tensor on the plan device')
        args.gate = gate.data_ptr()
        args.gate_value = int(gate_value)
    args.flags = flags
    args.x_src_fold = int(x_src_fold)
    args.x_outer_stride = int(x_outer_stride)
    if not tune:
        # the plan's preference (auto_schedule); the library falls back to
        # its own choice where the preferred family cannot serve the call
        tune = plan.default_tune
        if isinstance(tune, dict):
            tune = tune.get(mode)
        if tune:
            args.flags = flags | FLAG_TUNE_HINT
    if tune:
        for i, v in enumerate(tune):
            args.tune[i] = int(v)
    # (this sits in front of every variable of a Dataset: the device context
    # is entered only where the current device is another)
    _launch(torch, plan, lib.remap_apply_f64, 'remap_apply_f64', args,
            enter=torch.cuda.current_device() != plan.device.index)


#: An array a row pass reads by source cell, as :func:`_row_pass` is told of
#: it: its name in messages and in the argument struct, the tensor, and its
#: strides in elements (``outer`` goes with ``x_src_fold``).
_Source = collections.namedtuple('_Source',
                                 'name tensor row batch inner outer')


def _row_pass(args_type, entry, plan, reads, sources, results, own,
              *, n_batch, k_inner, y_row_stride, y_batch_stride, row_begin,
              row_end, x_src_fold, threshold=None, beside=(), limits=(),
              depth=None, csr=('rowptr', 'col', 'val'), strict=True):
    """
    What the launches beside the apply share, as ``rowpass::check_args``
    states it on the C side: their checks, the fields every ``remap_*_args``
    has, and the launch of ``entry`` with an ``args_type`` on torch's current
    stream.

    ``sources``: the :class:`_Source` arrays, the first of them the one the
    ``x_*`` fields describe; ``results``: ``(name, tensor)`` of the float64
    arrays addressed by destination row with the ``y_*`` strides.  Both go
    into the field of their name.  ``beside``: ``(name, tensor)`` of the
    pass's other arrays, which the device message names between the two;
    ``limits``: ``(name, tensor or None)`` of optional arrays addressed like
    the results.  ``depth``: the inner extent of the sources where it is not
    ``k_inner``.  ``own``: the fields that are the pass's alone.

    ``reads`` says why the plan must still hold the ``csr`` arrays.  The
    caller has refused a multi-device plan (:func:`_one_device`) before it
    looked at an array of its own.
    ``strict=False`` is the limiter's older contract: arrays need not be
    contiguous, and a launch without batches leaves the fold to the library.
    """
    torch = _torch()
    lib = load_library()
    arrays = [(s.name, s.tensor) for s in sources] + list(beside) + \
        list(results)
    for name, t in arrays:
        if t.device != plan.device:
            raise ValueError(', '.join(n for n, _ in arrays) +
                             ' and the plan must live on the same device')
        if strict and not t.is_contiguous():
            raise ValueError(f'{name} must be contiguous')
    if any(t.dtype != torch.float64 for _, t in results):
        raise TypeError(' and '.join(n for n, _ in results) +
                        ' must be float64')
    x = sources[0]
    x_dtype = _float_dtype(torch, x.name, x.tensor)
    row_begin, end = _row_range(plan, row_begin, row_end)
    if n_batch < 0 or k_inner < 0:
        raise ValueError('n_batch and k_inner must not be negative')
    if strict and x_src_fold:
        _check_fold(plan.n_a, x_src_fold, *(s.outer for s in sources))
    for s in sources:
        _check_reach(s.name, s.tensor, plan.n_a, s.row, s.batch, s.inner,
                     n_batch, k_inner if depth is None else depth,
                     x_src_fold, s.outer)
    for name, t in list(results) + list(limits):
        _check_reach(name, t, plan.n_b, y_row_stride, y_batch_stride, 1,
                     n_batch, k_inner)
    _holds_csr(plan, csr, reads)
    args = args_type()
    args.A = plan._csr_struct()
    args.row_begin = row_begin
    args.row_end = end
    args.x_dtype = x_dtype
    args.x_row_stride = int(x.row)
    args.x_batch_stride = int(x.batch)
    args.x_src_fold = int(x_src_fold)
    args.x_outer_stride = int(x.outer)
    args.y_row_stride = int(y_row_stride)
    args.y_batch_stride = int(y_batch_stride)
    args.n_batch = int(n_batch)
    args.k_inner = int(k_inner)
    if threshold is not None:
        args.threshold = float(threshold)
    for name, t in arrays:
        setattr(args, name, t.data_ptr())
    for name, value in own.items():
        setattr(args, name, value)
    _launch(torch, plan, getattr(lib, entry), entry, args)


def cotangent_strided(plan, X, Y, *, mode, n_batch, k_inner, x_row_stride,
                      x_batch_stride, y_row_stride, y_batch_stride,
                      threshold=0.0, row_begin=0, row_end=None, gate=None,
                      gate_value=0, x_src_fold=0, x_outer_stride=0):
    """
    One asynchronous launch of the cotangent of the division
    (``MODE_COTAN_FRACB`` / ``MODE_COTAN_MASKED`` of ``remap_apply_f64``,
    ``csrc/apply_cotangent.h``; :mod:`pyremap_amd.adjoint` has the definition
    to the bit) on torch's current stream.  ``Y`` (float64) holds the
    cotangent ``G`` of the forward's result on entry and ``T`` on exit,
    addressed with the forward's ``y_*`` strides; ``X`` is the forward's
    field (float64 or float32), read for NaN only with the forward's ``x_*``
    strides -- ``MODE_COTAN_FRACB`` does not read it and takes ``None``.  A
    row pass over the plan's own CSR: no schedule, no tune, one device; rows
    outside ``[row_begin, row_end)`` and a closed ``gate`` leave ``Y``
    untouched.
    """
    torch = _torch()
    lib = load_library()
    _one_device(plan, 'the cotangent of the division')
    if mode not in (MODE_COTAN_FRACB, MODE_COTAN_MASKED):
        raise ValueError(f'mode {mode} is no cotangent: expected '
                         f'MODE_COTAN_FRACB or MODE_COTAN_MASKED')
    masked = mode == MODE_COTAN_MASKED
    if masked and X is None:
        raise ValueError("MODE_COTAN_MASKED needs X, the forward's field")
    if not masked:
        X = None
    for name, t in (('X', X), ('Y', Y)):
        if t is not None and t.device != plan.device:
            raise ValueError('X, Y and the plan must live on the same device')
    if Y.dtype != torch.float64:
        raise TypeError('Y must be float64')
    x_dtype = DTYPE_F64 if X is None else _float_dtype(torch, 'X', X)
    row_begin, end = _row_range(plan, row_begin, row_end)
    if n_batch < 0 or k_inner < 0:
        raise ValueError('n_batch and k_inner must not be negative')
    if x_src_fold:
        _check_fold(plan.n_a, x_src_fold, x_outer_stride)
    _check_reach('X', X, plan.n_a, x_row_stride, x_batch_stride, 1, n_batch,
                 k_inner, x_src_fold, x_outer_stride)
    _check_reach('Y', Y, plan.n_b, y_row_stride, y_batch_stride, 1, n_batch,
                 k_inner)
    _holds_csr(plan, ('rowptr', 'col', 'val'),
               "the cotangent adds a row's weights from it")
    args = _ApplyArgs()
    args.A = plan._csr_struct()
    args.row_begin, args.row_end = row_begin, end
    args.X = X.data_ptr() if X is not None else None
    args.x_dtype, args.mode = x_dtype, mode
    args.x_row_stride = int(x_row_stride)
    args.x_batch_stride = int(x_batch_stride)
    args.Y = Y.data_ptr()
    args.y_row_stride = int(y_row_stride)
    args.y_batch_stride = int(y_batch_stride)
    args.n_batch, args.k_inner = int(n_batch), int(k_inner)
    args.frac_b = None if masked else plan.frac_b.data_ptr()
    args.threshold = float(threshold)
    if gate is not None:
        if gate.dtype != torch.int32 or gate.device != plan.device:
            raise TypeError('gate must be an int32 tensor on the plan device')
        args.gate = gate.data_ptr()
        args.gate_value = int(gate_value)
    args.x_src_fold = int(x_src_fold)
    args.x_outer_stride = int(x_outer_stride)
    _launch(torch, plan, lib.remap_apply_f64, 'remap_apply_f64', args)


def check_limiter(limiter):
    """``limiter`` is one of ``None | 'clip' | 'caas'``."""
    if limiter not in LIMITERS:
        raise ValueError(f"unknown limiter {limiter!r}: expected one of "
                         f"None, 'clip', 'caas'")
    return limiter


def limit_strided(plan, X, Y, *, n_batch, k_inner, x_row_stride,
                  x_batch_stride, y_row_stride, y_batch_stride, lo=None,
                  hi=None, row_begin=0, row_end=None, x_src_fold=0,
                  x_outer_stride=0):
    """
    One asynchronous ``remap_limit_rows`` launch on torch's current stream,
    after the apply launch that filled ``Y`` from ``X`` with the same strides
    (in elements): every ``Y[i, b, k]`` of rows ``[row_begin, row_end)`` is
    clamped, in place, to the bounds of the source values of row ``i``'s
    stored entries (:mod:`pyremap_amd.limiter` has the semantics).  ``lo`` /
    ``hi``: optional float64 device tensors addressed like ``Y`` that receive
    the bounds.

    The pass reads the plan's own CSR (``rowptr``, ``col``), never a
    schedule: a plan applied as short and long rows (``plan._split``) is
    limited as the one matrix it is, a row slice over its own rows.
    """
    torch = _torch()
    _one_device(plan, 'the limiter')
    for name, t in (('lo', lo), ('hi', hi)):
        if t is not None and (t.dtype != torch.float64 or
                              t.device != plan.device):
            raise TypeError(f'{name} must be a float64 tensor on the plan '
                            f'device')
    _row_pass(
        _LimitArgs, 'remap_limit_rows', plan,
        "the limiter gathers a row's sources from it",
        [_Source('X', X, x_row_stride, x_batch_stride, 1, x_outer_stride)],
        [('Y', Y)], dict(lo=_ptr(lo), hi=_ptr(hi)),
        n_batch=n_batch, k_inner=k_inner, y_row_stride=y_row_stride,
        y_batch_stride=y_batch_stride, row_begin=row_begin, row_end=row_end,
        x_src_fold=x_src_fold, limits=(('lo', lo), ('hi', hi)),
        csr=('rowptr', 'col'), strict=False)


def _caas_mass(Yv, row_weight):
    """``sum_V w_i y_i`` per column of the ``(n_batch, n_b, k_inner)`` view
    ``Yv``, V the rows whose value is no NaN."""
    torch = _torch()
    w = row_weight.view(1, -1, 1)
    return torch.where(torch.isnan(Yv), 0.0, w * Yv).sum(dim=1)


def _caas_fixup(Yv, M, lo, hi, row_weight):
    """
    The second half of "clip and assured sum" (``limiter.caas`` is the
    statement), in place on the clipped ``(n_batch, n_b, k_inner)`` view
    ``Yv`` with the bounds ``lo`` / ``hi`` of the same view and ``M`` the
    mass of the unlimited result (:func:`_caas_mass`, taken before the clip).
    Device tensor operations, nothing is read back.  Where the bounds cannot
    hold the mass every value goes to its bound and conservation is not
    reached.
    """
    torch = _torch()
    w = row_weight.view(1, -1, 1)
    valid = ~torch.isnan(Yv)
    Mc = torch.where(valid, w * Yv, 0.0).sum(dim=1)
    dM = M - Mc
    up = (dM > 0).unsqueeze(1)
    cap = torch.where(up, hi - Yv, Yv - lo)
    bound = torch.where(up, hi, lo)
    C = torch.where(valid, w * cap, 0.0).sum(dim=1)
    ok = torch.isfinite(M) & torch.isfinite(Mc) & torch.isfinite(C) & \
        (C > 0) & (dM != 0)
    t = torch.where(ok, dM.abs() / C, 0.0)
    full = (ok & (t >= 1)).unsqueeze(1)
    step = torch.where(dM > 0, t, -t).unsqueeze(1)
    new = torch.maximum(torch.minimum(Yv + step * cap, hi), lo)
    new = torch.where(full, bound, new)
    Yv.copy_(torch.where(ok.unsqueeze(1) & valid, new, Yv))


def _limit_views(t, n_batch, n_b, k_inner, y_row_stride, y_batch_stride):
    """The ``(n_batch, n_b, k_inner)`` strided view of a result buffer."""
    return t.as_strided((n_batch, n_b, k_inner),
                        (y_batch_stride, y_row_stride, 1),
                        t.storage_offset())


def _limit_after_apply(plan, limiter, row_weight, X, Y, **strides):
    """Clip -- and, for CAAS, hand the clipped mass back -- behind the apply
    launch that filled the contiguous buffer ``Y``.  CAAS takes two scratch
    tensors of ``Y``'s size for the bounds."""
    torch = _torch()
    if limiter == 'clip':
        limit_strided(plan, X, Y, **strides)
        return
    view = (strides['n_batch'], plan.n_b, strides['k_inner'],
            strides['y_row_stride'], strides['y_batch_stride'])
    Yv = _limit_views(Y.view(-1), *view)
    M = _caas_mass(Yv, row_weight)       # of the unlimited result
    lo = torch.empty(Y.numel(), dtype=torch.float64, device=Y.device)
    hi = torch.empty(Y.numel(), dtype=torch.float64, device=Y.device)
    limit_strided(plan, X, Y, lo=lo, hi=hi, **strides)
    _caas_fixup(Yv, M, _limit_views(lo, *view), _limit_views(hi, *view),
                row_weight)


def _limiter_arguments(plan, limiter, row_weight):
    """The checks of ``limiter=`` / ``row_weight=`` in front of any launch;
    returns the float64 device weights (None unless CAAS)."""
    check_limiter(limiter)
    if limiter is None:
        return None
    _one_device(plan, 'the limiter')
    if limiter != 'caas':
        return None
    if row_weight is None:
        raise ValueError("limiter 'caas' needs row_weight (one weight per "
                         'destination row: area_b * frac_b)')
    torch = _torch()
    w = torch.as_tensor(row_weight).to(device=plan.device,
                                       dtype=torch.float64).contiguous()
    if tuple(w.shape) != (plan.n_b,):
        raise ValueError(f'row_weight of shape {tuple(w.shape)}: expected '
                         f'({plan.n_b},)')
    return w


def sgs_strided(plan, X, F, Y, *, n_batch, k_inner, x_row_stride,
                x_batch_stride, f_row_stride, f_batch_stride, f_inner_stride,
                y_row_stride, y_batch_stride, threshold, row_begin=0,
                row_end=None, x_src_fold=0, x_outer_stride=0,
                f_outer_stride=0):
    """
    One asynchronous ``remap_apply_sgs`` launch on torch's current stream:
    the sub-gridscale weighted remap of ``X`` by the fraction ``F`` into rows
    ``[row_begin, row_end)`` of ``Y`` (:mod:`pyremap_amd.sgs` has the
    semantics; strides in elements).  ``X`` and ``Y`` are addressed as
    :func:`apply_strided` addresses them, ``F`` like ``X`` with strides of its
    own: ``f_batch_stride == 0`` broadcasts over the batches,
    ``f_inner_stride`` (0 or 1) ``== 0`` over the inner index;
    ``f_outer_stride`` goes with ``x_src_fold``.

    The launch reads the plan's own CSR (``rowptr``, ``col``, ``val``), never
    a schedule: a plan applied as short and long rows (``plan._split``) is
    served as the one matrix it is.
    """
    _one_device(plan, 'sub-gridscale weighting')
    f_dtype = _float_dtype(_torch(), 'F', F)
    if f_inner_stride not in (0, 1):
        raise ValueError(f'f_inner_stride {f_inner_stride}: expected 0 '
                         f'(broadcast) or 1')
    _row_pass(
        _SgsArgs, 'remap_apply_sgs', plan,
        'the sub-gridscale launch reads it',
        [_Source('X', X, x_row_stride, x_batch_stride, 1, x_outer_stride),
         _Source('F', F, f_row_stride, f_batch_stride, f_inner_stride,
                 f_outer_stride)],
        [('Y', Y)],
        dict(f_dtype=f_dtype, f_row_stride=int(f_row_stride),
             f_batch_stride=int(f_batch_stride),
             f_inner_stride=int(f_inner_stride),
             f_outer_stride=int(f_outer_stride)),
        n_batch=n_batch, k_inner=k_inner, y_row_stride=y_row_stride,
        y_batch_stride=y_batch_stride, row_begin=row_begin, row_end=row_end,
        x_src_fold=x_src_fold, threshold=threshold)


#: A column pass (csrc/colpass.h) as :func:`_columns_strided` is told of it:
#: the argument struct and the entry point; the companion array and the array
#: of what is asked for, as messages and the struct's fields name them (the
#: companion's other fields carry its name in lower case); the numbers asked
#: for per output and what messages call them; the pass in words.
_ColumnPass = collections.namedtuple(
    '_ColumnPass', 'args entry companion query per_output numbers activity')
_LEVELS = _ColumnPass(_LevelsArgs, 'remap_apply_levels', 'Z', 'T', 1,
                      'targets', 'the level interpolation')
_LAYERS = _ColumnPass(_LayersArgs, 'remap_apply_layers', 'H', 'bounds', 2,
                      'numbers', 'the layer reduction')


def _columns_strided(cp, plan, X, C, Q, Y, *, n_batch, n_levels, k_inner,
                     x_row_stride, x_batch_stride, c_row_stride,
                     c_batch_stride, y_row_stride, y_batch_stride, threshold,
                     row_begin=0, row_end=None, x_src_fold=0,
                     x_outer_stride=0, c_outer_stride=0, **own):
    """What :func:`levels_strided` and :func:`layers_strided` share: one
    launch of the column pass ``cp`` with the companion ``C``, its strides
    under the names ``c_*``, and the outputs' ``Q``.  ``own``: the fields of
    the argument struct that are the pass's alone."""
    torch = _torch()
    _one_device(plan, cp.activity)
    if Q.dtype != torch.float64:
        raise TypeError(f'{cp.query} must be float64')
    c = cp.companion.lower()
    own[c + '_dtype'] = _float_dtype(torch, cp.companion, C)
    if n_levels < 1:
        raise ValueError(f'n_levels {n_levels}: expected >= 1')
    if Q.numel() < cp.per_output * k_inner:
        raise ValueError(f'{cp.query} holds {Q.numel()} {cp.numbers}; '
                         f'k_inner is {k_inner}')
    own.update({'n_levels': int(n_levels),
                c + '_row_stride': int(c_row_stride),
                c + '_batch_stride': int(c_batch_stride),
                c + '_outer_stride': int(c_outer_stride)})
    _row_pass(
        cp.args, cp.entry, plan, cp.activity + ' reads it',
        [_Source('X', X, x_row_stride, x_batch_stride, 1, x_outer_stride),
         _Source(cp.companion, C, c_row_stride, c_batch_stride, 1,
                 c_outer_stride)],
        [('Y', Y)], own, beside=[(cp.query, Q)],
        n_batch=n_batch, k_inner=k_inner, y_row_stride=y_row_stride,
        y_batch_stride=y_batch_stride, row_begin=row_begin, row_end=row_end,
        x_src_fold=x_src_fold, threshold=threshold,
        # (a launch without batches or outputs reads nothing; one with them
        # reads whole columns)
        depth=n_levels if k_inner > 0 else 0)


def levels_strided(plan, X, Z, T, Y, *, n_batch, n_levels, k_inner,
                   x_row_stride, x_batch_stride, z_row_stride,
                   z_batch_stride, y_row_stride, y_batch_stride, threshold,
                   row_begin=0, row_end=None, x_src_fold=0, x_outer_stride=0,
                   z_outer_stride=0):
    """
    One asynchronous ``remap_apply_levels`` launch on torch's current stream:
    every entry of a row interpolates its source column ``X[cell, b, :]`` on
    the level coordinate ``Z[cell, b', :]`` (``n_levels`` each, stride 1) to
    the ``k_inner`` targets ``T`` and enters the masked, renormalised sum of
    rows ``[row_begin, row_end)`` of ``Y`` (:mod:`pyremap_amd.levels` has the
    semantics; strides in elements).  ``X`` and ``Y`` are addressed as
    :func:`apply_strided` addresses them, with ``n_levels`` the inner extent
    of ``X`` and ``k_inner`` that of ``Y``; ``Z`` like ``X`` with strides of
    its own: ``z_row_stride == 0`` is one coordinate for all cells,
    ``z_batch_stride == 0`` a time-invariant one; ``z_outer_stride`` goes
    with ``x_src_fold``.  ``T``: a float64 device tensor of ``k_inner``
    targets, in any order.

    The launch reads the plan's own CSR (``rowptr``, ``col``, ``val``), never
    a schedule: a plan applied as short and long rows (``plan._split``) is
    served as the one matrix it is.
    """
    _columns_strided(
        _LEVELS, plan, X, Z, T, Y, n_batch=n_batch, n_levels=n_levels,
        k_inner=k_inner, x_row_stride=x_row_stride,
        x_batch_stride=x_batch_stride, c_row_stride=z_row_stride,
        c_batch_stride=z_batch_stride, y_row_stride=y_row_stride,
        y_batch_stride=y_batch_stride, threshold=threshold,
        row_begin=row_begin, row_end=row_end, x_src_fold=x_src_fold,
        x_outer_stride=x_outer_stride, c_outer_stride=z_outer_stride)


def layers_strided(plan, X, H, bounds, Y, *, n_batch, n_levels, k_inner,
                   x_row_stride, x_batch_stride, h_row_stride,
                   h_batch_stride, y_row_stride, y_batch_stride, threshold,
                   reduce='mean', row_begin=0, row_end=None, x_src_fold=0,
                   x_outer_stride=0, h_outer_stride=0):
    """
    One asynchronous ``remap_apply_layers`` launch on torch's current stream:
    every entry of a row reduces its source column ``X[cell, b, :]`` with the
    layer thicknesses ``H[cell, b', :]`` (``n_levels`` each, stride 1) over
    the ``k_inner`` depth ranges ``bounds`` -- the thickness-weighted mean
    (``reduce='mean'``) or the integral (``'integral'``) -- and enters the
    masked, renormalised sum of rows ``[row_begin, row_end)`` of ``Y``
    (:mod:`pyremap_amd.layers` has the semantics; strides in elements).
    ``X``, ``Y`` and ``H`` are addressed as :func:`levels_strided` addresses
    ``X``, ``Y`` and ``Z``: ``h_row_stride == 0`` is one thickness column for
    all cells, ``h_batch_stride == 0`` a time-invariant thickness;
    ``h_outer_stride`` goes with ``x_src_fold``.  ``bounds``: a float64
    device tensor of ``2 * k_inner`` numbers, ``A_0, B_0, A_1, ...``.

    The launch reads the plan's own CSR (``rowptr``, ``col``, ``val``), never
    a schedule.
    """
    _one_device(plan, _LAYERS.activity)
    _columns_strided(
        _LAYERS, plan, X, H, bounds, Y, n_batch=n_batch, n_levels=n_levels,
        k_inner=k_inner, x_row_stride=x_row_stride,
        x_batch_stride=x_batch_stride, c_row_stride=h_row_stride,
        c_batch_stride=h_batch_stride, y_row_stride=y_row_stride,
        y_batch_stride=y_batch_stride, threshold=threshold,
        row_begin=row_begin, row_end=row_end, x_src_fold=x_src_fold,
        x_outer_stride=x_outer_stride, c_outer_stride=h_outer_stride,
        reduce=_reduce_code(reduce))


def _check_basis(torch, name, B, rows):
    """A basis of the vector launch: a contiguous float64 ``(rows, 5)``
    tensor (:func:`_row_pass` holds it to the plan's device)."""
    if B.dtype != torch.float64:
        raise TypeError(f'{name} must be float64')
    if tuple(B.shape) != (rows, 5) or not B.is_contiguous():
        raise ValueError(f'{name} of shape {tuple(B.shape)}: expected a '
                         f'contiguous ({rows}, 5)')


def vector_strided(plan, U, V, BA, BB, YU, YV, *, n_batch, k_inner,
                   x_row_stride, x_batch_stride, y_row_stride,
                   y_batch_stride, threshold, row_begin=0, row_end=None,
                   x_src_fold=0, x_outer_stride=0):
    """
    One asynchronous ``remap_apply_vector`` launch on torch's current stream:
    the eastward and northward components ``U`` and ``V`` are rotated to
    Cartesian with the source basis ``BA (n_a, 5)``, summed with the rows'
    weights and projected on the destination basis ``BB (n_b, 5)`` into rows
    ``[row_begin, row_end)`` of ``YU`` and ``YV`` (:mod:`pyremap_amd.vector`
    has the semantics; strides in elements).  ``U`` and ``V`` share one
    dtype and one set of strides, addressed as :func:`apply_strided`
    addresses ``X``; ``YU`` and ``YV`` share the strides of ``Y``.

    The launch reads the plan's own CSR (``rowptr``, ``col``, ``val``), never
    a schedule: a plan applied as short and long rows (``plan._split``) is
    served as the one matrix it is.
    """
    torch = _torch()
    _one_device(plan, 'the vector remap')
    _float_dtype(torch, 'U', U)
    if V.dtype != U.dtype:
        raise TypeError(f'U and V must have one dtype, not {U.dtype} and '
                        f'{V.dtype}')
    _check_basis(torch, 'BA', BA, plan.n_a)
    _check_basis(torch, 'BB', BB, plan.n_b)
    _row_pass(
        _VectorArgs, 'remap_apply_vector', plan,
        'the vector launch reads it',
        [_Source(name, t, x_row_stride, x_batch_stride, 1, x_outer_stride)
         for name, t in (('U', U), ('V', V))],
        [('YU', YU), ('YV', YV)], {}, beside=[('BA', BA), ('BB', BB)],
        n_batch=n_batch, k_inner=k_inner, y_row_stride=y_row_stride,
        y_batch_stride=y_batch_stride, row_begin=row_begin, row_end=row_end,
        x_src_fold=x_src_fold, threshold=threshold)


def _prod(seq):
    out = 1
    for s in seq:
        out *= int(s)
    return out


def in_place_addressable(shape, remap_axes):
    """
    Can a field of this shape be addressed in place (strides instead of
    permute copies)?  The source axes must be adjacent -- then every layout
    has its kernel: a run of >= 8 contiguous fields behind the source axes
    goes to the lanes-across-K kernels, shorter runs in several batches
    ((Time, nCells), the reference's most common input) to the
    lanes-across-rows kernel (``spmm_rowcell``), K <= 32 to the
    lane-per-(row, k) kernel.
    """
    ndim = len(shape)
    axes = [int(a) % ndim for a in remap_axes]
    lead = min(axes)
    return axes == list(range(lead, lead + len(axes)))


def check_field_extents(n_a, n_b, n_b_global, dst_grid_dims, shape,
                        remap_axes):
    """
    The contract between a field and a mapping, stated once: the axes
    ``remap_axes`` of a field of shape ``shape`` hold exactly ``n_a`` source
    cells, and ``dst_grid_dims`` (C order; ``None``: flat rows) holds exactly
    ``n_b`` cells.  A row shard (``n_b != n_b_global``) answers with its flat
    slab of rows, so its ``dst_grid_dims`` -- the grid of the WHOLE mapping --
    is not compared.  Raises ``ValueError``; returns ``(axes, dst_shape)``:
    the axes made non-negative and the destination dims of the result.

    Everything behind this check addresses raw pointers with ``n_a`` and
    ``n_b``: every route to a launch or a 2-D copy calls it before its first
    allocation, stream wait, thread, copy or launch.
    """
    # (plain loops: this runs in front of every launch, microseconds count)
    ndim = len(shape)
    axes = [int(a) % ndim for a in remap_axes]
    n_src = 1
    for ax in axes:
        n_src *= int(shape[ax])
    if n_src != n_a:
        raise ValueError(
            f'the remapped axes hold {n_src} source cells but the mapping '
            f'has n_a = {n_a}')
    # rows stay flat for a shard (its rows are no whole grid) and when the
    # caller names no destination grid
    if dst_grid_dims is None or n_b != n_b_global:
        return axes, [int(n_b)]
    dst_shape = [int(d) for d in dst_grid_dims]
    n_dst = 1
    for d in dst_shape:
        n_dst *= d
    if n_dst != n_b:
        raise ValueError(f'dst_grid_dims {dst_shape} do not hold n_b = '
                         f'{n_b} cells')
    return axes, dst_shape


#: How a field is laid out for its launches (:func:`field_layout`).
#:   route      'direct' | 'fold' | 'permute'
#:   order      None: X is the contiguous field; else X is the field permuted
#:              by ``order`` and flattened to ``(n_a, K)``
#:   y_shape    shape of the float64 buffer the launches write
#:   out_shape  shape of the caller's result
#:   n_launch   launches; launch ``li`` takes row ``li`` of X and of the
#:              buffer, each reshaped to ``(n_launch, -1)``
#:   strides    the keywords every launch has in common: ``n_batch``,
#:              ``k_inner``, the X and Y strides and, on the 'fold' route,
#:              ``x_src_fold`` and ``x_outer_stride``
#:   groups     the field's other axes as ``(lead, between, tail)``: the
#:              launches, the batches and the inner index on the 'fold'
#:              route; the batches, none and the inner index on 'direct';
#:              on 'permute' all of them are ``tail``
#:   back       None: the buffer is the result; else ``(shape, unpermute)``:
#:              the buffer reshaped and permuted is
FieldLayout = collections.namedtuple(
    'FieldLayout', 'route order y_shape out_shape n_launch strides groups '
                   'back')


def field_layout(plan, shape, remap_axes, dst_shape, fold=True):
    """
    The one statement of how a field of ``shape`` whose (non-negative) axes
    ``remap_axes`` hold the source grid is addressed by the launches, and how
    their buffer becomes the result with ``dst_shape`` at ``min(remap_axes)``
    (``remap_numpy.py:254-256`` and ``:280-295``).  Pure shape arithmetic.

    'direct'   source axes adjacent: addressed in place, strides do the
               permute and the flatten;
    'fold'     two source axes with other dims BETWEEN them -- (lat, M, lon[,
               T]) -- in place too: the dims between are the batches of the
               launch, a source cell is addressed through two strides
               (``x_src_fold``), one launch per index of the dims in front
               (``fold=False``: not taken);
    'permute'  general axis order: one device transpose to ``(n_a, K)``, the
               kernel, one transpose back.
    """
    # (the in-place route first, with nothing worked out that it does not
    # need: it sits in front of every variable of a Dataset)
    ndim = len(shape)
    lead = min(remap_axes)
    end = lead + len(remap_axes)
    if remap_axes == list(range(lead, end)):    # (in_place_addressable)
        lead_shape = [int(s) for s in shape[:lead]]
        tail_shape = [int(s) for s in shape[end:]]
        k_inner = _prod(tail_shape)
        out_shape = lead_shape + dst_shape + tail_shape
        strides = dict(n_batch=_prod(lead_shape), k_inner=k_inner,
                       x_row_stride=k_inner,
                       x_batch_stride=plan.n_a * k_inner,
                       y_row_stride=k_inner,
                       y_batch_stride=plan.n_b * k_inner)
        groups = (range(lead), (), range(end, ndim))
        return FieldLayout('direct', None, out_shape, out_shape, 1, strides,
                           groups, None)
    shape = [int(s) for s in shape]
    extra_axes = [ax for ax in range(ndim) if ax not in remap_axes]
    out_shape = shape[:lead] + dst_shape + \
        [shape[ax] for ax in extra_axes if ax > lead]
    if fold and len(remap_axes) == 2 and remap_axes[0] < remap_axes[1]:
        a0, a1 = remap_axes
        nx = shape[a1]
        M = _prod(shape[a0 + 1:a1])
        T = _prod(shape[a1 + 1:])
        strides = dict(n_batch=M, k_inner=T, x_row_stride=T,
                       x_batch_stride=nx * T, y_row_stride=M * T,
                       y_batch_stride=T, x_src_fold=nx,
                       x_outer_stride=M * nx * T)
        groups = (range(a0), range(a0 + 1, a1), range(a1 + 1, ndim))
        return FieldLayout('fold', None, out_shape, out_shape,
                           _prod(shape[:a0]), strides, groups, None)
    K = _prod(shape[ax] for ax in extra_axes)
    strides = dict(n_batch=1, k_inner=K, x_row_stride=K, x_batch_stride=0,
                   y_row_stride=K, y_batch_stride=0)
    n_dst = len(dst_shape)
    tail = list(range(n_dst, n_dst + len(extra_axes)))
    unpermute = tail[:lead] + list(range(n_dst)) + tail[lead:]
    back = (dst_shape + [shape[ax] for ax in extra_axes], unpermute)
    return FieldLayout('permute', remap_axes + extra_axes, [plan.n_b, K],
                       out_shape, 1, strides, ((), (), extra_axes), back)


def _launch_source(plan, lay, t, k):
    """``t`` (the field, or what is laid out like it) as the launches read
    it: contiguous, or permuted to ``(n_a, k)``."""
    if lay.order is None:
        return t.contiguous()
    return t.permute(lay.order).reshape(plan.n_a, k).contiguous()


def _launch_rows(n, *tensors):
    """Per launch, the contiguous piece of each tensor (None stays None)."""
    if n == 1:
        return [tensors]
    rows = [None if t is None else t.reshape(n, t.numel() // n if n else 0)
            for t in tensors]
    return [[None if r is None else r[li] for r in rows] for li in range(n)]


def _launch_result(lay, t):
    if lay.back is None:
        return t
    shape, unpermute = lay.back
    return t.reshape(shape).permute(unpermute).contiguous()


def remap_tensor(plan, dst_grid_dims, field, remap_axes, mode, threshold=0.0,
                 want_mask=False, flags=0, tune=None, out=None, gate=None,
                 gate_value=0, mask_out=None, limiter=None, row_weight=None):
    """
    Device-level ``_remap_numpy_array``: ``field`` is a device tensor whose
    axes ``remap_axes`` hold the source grid; returns the float64 tensor with
    those axes replaced by ``dst_grid_dims`` at ``min(remap_axes)``
    (``remap_numpy.py:280-295``), NaN where the reference masks, and the
    uint8 mask (1 = masked) when ``want_mask``.

    ``dst_grid_dims`` is in C order; for a row shard the leading destination
    dimension is replaced by the shard's row count (the result is the flat
    slab of rows ``[plan.row_offset, plan.row_offset + plan.n_b)``).

    ``mode=MODE_LAF``: largest area fraction for labels
    (:mod:`pyremap_amd.laf`) -- float64 too, same layout, NaN where no class
    exists or ``valid <= threshold``; one device, never limited; ``flags``
    and ``tune`` are ignored.  ``MODE_MIN``, ``MODE_MAX``, ``MODE_VAR`` and
    ``MODE_MEDIAN``: sub-grid statistics (:mod:`pyremap_amd.rowstat`), under
    the same terms.

    ``limiter`` (``None | 'clip' | 'caas'``; :mod:`pyremap_amd.limiter`):
    after the apply, on the same stream, every value is clamped to the bounds
    of the source values of its row's entries (``remap_limit_rows``; whatever
    the mode left is what is limited, NaN stays NaN); ``'caas'`` then hands
    the clipped mass back within the bounds so that ``sum_i row_weight[i] *
    y[i]`` of every column is what it was (``row_weight``: ``n_b`` weights
    ``>= 0``, ``area_b * frac_b`` for a conservative map).  Where the bounds
    cannot hold the mass every value ends on its bound and conservation is
    not reached; nothing reports it.  CAAS takes two scratch tensors of the
    result's size.  A gated launch is not limited (the limiter needs no
    gate: ``remap_tensor_auto_mode`` runs it once behind its launches).
    """
    torch = _torch()
    weight = _limiter_arguments(plan, limiter, row_weight)
    if limiter is not None and gate is not None:
        raise ValueError('a gated launch is not limited: run the limiter '
                         'behind the gated launches')
    if mode == MODE_LAF:
        # labels: every value is a source value of its own row already
        if limiter is not None:
            raise ValueError('largest area fraction is not limited: its '
                             'values are source values of their own rows')
        _one_device(plan, 'largest area fraction')
    elif mode == MODE_CLASSFRAC:
        raise ValueError('class fractions have one more axis than the field: '
                         'remap_tensor_fractions lays them out')
    elif mode in _ROW_PASS_MODES:
        # what a limiter clamps to are the bounds of a mean
        if limiter is not None:
            raise ValueError('a row statistic is not limited: the bounds of '
                             'a row are no bounds of its spread')
        _one_device(plan, _ROW_PASS_MODES[mode])
    if hasattr(plan, 'shards'):
        # a parallel.MultiDeviceRemap standing where the plan stands
        # (Remapper(..., devices=[...])): rows sharded over several GPUs
        if out is not None or gate is not None or mask_out is not None or \
                tune is not None:
            raise ValueError('out / gate / mask_out / tune address ONE '
                             "device's launch; not with a multi-device plan")
        return plan.remap_tensor(dst_grid_dims, field, remap_axes, mode,
                                 threshold=threshold, want_mask=want_mask,
                                 flags=flags)
    remap_axes, dst_shape = check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_grid_dims, field.shape,
        remap_axes)
    if field.dtype not in (torch.float64, torch.float32):
        # scipy upcasts everything else to float64 before the product
        field = field.to(torch.float64)
    lay = field_layout(plan, field.shape, remap_axes, dst_shape,
                       fold=out is None and gate is None and mask_out is None)
    direct = lay.route == 'direct'
    out_shape = lay.out_shape
    if out is not None:
        # the kernel writes through out.data_ptr(): anything but a float64,
        # contiguous tensor of exactly the result's shape on the plan's
        # device would be an out-of-bounds device write
        if out.dtype != torch.float64 or out.device != plan.device or \
                tuple(out.shape) != tuple(out_shape) or \
                not out.is_contiguous():
            raise ValueError(
                f'out must be a contiguous float64 tensor of shape '
                f'{tuple(out_shape)} on {plan.device}, got '
                f'{out.dtype} {tuple(out.shape)} on {out.device}')

    if mask_out is not None and (
            mask_out.dtype != torch.uint8 or mask_out.device != plan.device or
            tuple(mask_out.shape) != tuple(out_shape) or
            not mask_out.is_contiguous()):
        raise ValueError(
            f'mask_out must be a contiguous uint8 tensor of shape '
            f'{tuple(out_shape)} on {plan.device}')
    if not direct and (gate is not None or mask_out is not None):
        raise ValueError('gated launches and caller-supplied masks need the '
                         'source axes adjacent (in-place addressing)')

    X = _launch_source(plan, lay, field, lay.strides['k_inner'])
    Y = out if direct and out is not None else torch.empty(
        lay.y_shape, dtype=torch.float64, device=field.device)
    mask = None
    if want_mask:
        mask = mask_out if mask_out is not None else torch.empty(
            lay.y_shape, dtype=torch.uint8, device=field.device)
    gated = dict(gate=gate, gate_value=gate_value) if direct else {}
    for Xl, Yl, Ml in _launch_rows(lay.n_launch, X, Y, mask):
        apply_strided(plan, Xl, Yl, mode=mode, threshold=threshold,
                      mask_out=Ml, flags=flags, tune=tune, **gated,
                      **lay.strides)
        if limiter is not None:
            # (on the launch's own buffer: before any transpose back)
            _limit_after_apply(plan, limiter, weight, Xl, Yl, **lay.strides)
    if lay.back is not None:
        Y = _launch_result(lay, Y)
        if out is not None:
            out.copy_(Y)
            Y = out
    return (Y, _launch_result(lay, mask)) if want_mask else Y


def _ascending_tensor(torch, values, device, check):
    """``values`` (a sequence, an array or a tensor) through ``check`` of
    :mod:`pyremap_amd.classfrac` as a float64 tensor on ``device``."""
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    return torch.from_numpy(check(values)).to(device)


def _label_source(torch, values):
    if not isinstance(values, torch.Tensor):
        raise TypeError('values must be a tensor (pyremap_amd.classfrac has '
                        'the numpy twins)')
    return values.to(torch.float64)


def class_labels(values, classes):
    """:func:`pyremap_amd.classfrac.labels_from_classes` on a tensor: the
    index of every value in the strictly ascending ``classes`` as float32
    (indices up to 256 are exact), -1 for a value that is not listed, NaN
    stays NaN."""
    from pyremap_amd import classfrac
    torch = _torch()
    v = _label_source(torch, values)
    c = _ascending_tensor(torch, classes, v.device, classfrac.check_classes)
    idx = torch.searchsorted(c, v.contiguous()).clamp_(max=c.numel() - 1)
    out = torch.where(c[idx] == v, idx.to(torch.float32),
                      torch.full((), -1.0, dtype=torch.float32,
                                 device=v.device))
    return torch.where(torch.isnan(v), torch.full_like(out, float('nan')),
                       out)


def bin_labels(values, edges):
    """:func:`pyremap_amd.classfrac.labels_from_bins` on a tensor: the bin of
    every value as float32, bin ``c`` being ``edges[c] <= x < edges[c + 1]``
    (+-inf edges allowed), -1 outside the edges, NaN stays NaN."""
    from pyremap_amd import classfrac
    torch = _torch()
    v = _label_source(torch, values)
    e = _ascending_tensor(torch, edges, v.device, classfrac.check_edges)
    idx = torch.searchsorted(e, v.contiguous(), right=True) - 1
    inside = (idx >= 0) & (idx < e.numel() - 1)
    out = torch.where(inside, idx.to(torch.float32),
                      torch.full((), -1.0, dtype=torch.float32,
                                 device=v.device))
    return torch.where(torch.isnan(v), torch.full_like(out, float('nan')),
                       out)


def remap_tensor_fractions(plan, dst_grid_dims, labels, n_classes, remap_axes,
                           threshold=0.0, want_mask=False):
    """
    Class (or bin) area fractions of a field of labels
    (:mod:`pyremap_amd.classfrac`; ``MODE_CLASSFRAC``): ``labels`` is a device
    tensor of class indices held as numbers (:func:`class_labels`,
    :func:`bin_labels`; NaN is missing, anything that is no integer in ``[0,
    n_classes)`` counts in the denominator alone) whose axes ``remap_axes``
    hold the source grid.  Returns the float64 tensor of shape ``(n_classes,)
    +`` the shape :func:`remap_tensor` would give, NaN where ``valid <=
    threshold``, and the uint8 mask (1 = masked) of that shape when
    ``want_mask``.

    The labels are gathered once per tile of 16 classes, not once per class.
    Dims in front of adjacent source axes (Time) are served by one launch
    each, dims behind them are the contiguous run of the launch; any other
    axis order is permuted to ``(n_a, K)`` first.  One device, never limited.
    """
    from pyremap_amd import classfrac
    torch = _torch()
    _one_device(plan, _ROW_PASS_MODES[MODE_CLASSFRAC])
    C = classfrac.check_n_classes(n_classes)
    remap_axes, dst_shape = check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_grid_dims, labels.shape,
        remap_axes)
    if labels.dtype not in (torch.float64, torch.float32):
        labels = labels.to(torch.float64)
    lay = field_layout(plan, labels.shape, remap_axes, dst_shape, fold=False)
    # 'direct': the dims in front are launches here (X is ONE batch)
    n_launch = lay.strides['n_batch']
    k = lay.strides['k_inner']
    X = _launch_source(plan, lay, labels, k)
    Y = torch.empty([C] + list(lay.y_shape), dtype=torch.float64,
                    device=labels.device)
    mask = torch.empty(Y.shape, dtype=torch.uint8, device=labels.device) \
        if want_mask else None
    piece = plan.n_b * k
    strides = dict(n_batch=C, k_inner=k, x_row_stride=k, x_batch_stride=0,
                   y_row_stride=k, y_batch_stride=n_launch * piece)
    if Y.numel():
        Xs = X.reshape(n_launch, plan.n_a * k)
        for li in range(n_launch):
            # launch li writes Y[:, li]: its own piece of every class
            apply_strided(
                plan, Xs[li], Y.reshape(-1)[li * piece:],
                mode=MODE_CLASSFRAC, threshold=threshold,
                mask_out=None if mask is None else
                mask.reshape(-1)[li * piece:], **strides)
    if lay.back is not None:
        shape, unpermute = lay.back
        order = [0] + [u + 1 for u in unpermute]
        Y = Y.reshape([C] + list(shape)).permute(order).contiguous()
        if mask is not None:
            mask = mask.reshape([C] + list(shape)).permute(order).contiguous()
    return (Y, mask) if want_mask else Y


def fill_tensor(plan, field, axes, method='nearest', passes=None,
                threshold=0.0, info=None):
    """
    Fill the missing (NaN) elements of ``field`` from their valid neighbours
    (:mod:`pyremap_amd.fill` has the definition to the bit): ``plan`` is the
    neighbour plan of ONE grid (``RemapPlan.from_triplets`` of
    :func:`pyremap_amd.fill.neighbour_graph`; square), ``field`` a float64 or
    float32 device tensor whose axes ``axes`` hold that grid.  Returns a new
    float64 tensor of the field's shape, detached from it.

    ``method``: ``'nearest'`` (``MODE_FILL_BEST``: the value of the valid
    neighbour with the largest weight; only values the field holds come out)
    or ``'mean'`` (``MODE_FILL_MEAN``: the weighted mean of the valid
    neighbours, ``threshold`` on their weight).  One pass fills one ring of
    cells; the pass is repeated between two buffers, the first one reading
    the field as it is (float32 too), every later one the float64 result.

    ``passes=k`` makes exactly ``k`` launches and never synchronises.
    ``passes=None`` repeats until a pass leaves the number of missing
    elements unchanged, zero included.  The count comes from the launch's
    ``mask_out`` and reading it back is the only synchronisation.  A pass
    that fills nothing is the identity, so the count is looked at only every
    ``FILL_CHECK_EVERY`` passes, and the result is still the one defined by
    "repeat until nothing changes": the passes launched beyond the last one
    that filled something change no byte.  A component of the graph with no
    valid value in some column stays NaN there.

    Axes that are adjacent and ascending are addressed in place: the dims in
    front are the batches of the launch, the dims behind its contiguous run.
    Any other order is permuted to ``(n, K)`` first and back afterwards.
    ``info``: a dict that receives ``passes`` (launches made) and, with
    ``passes=None``, ``missing`` (elements left).  One device.
    """
    from pyremap_amd import fill as fill_statement
    torch = _torch()
    _one_device(plan, _ROW_PASS_MODES[MODE_FILL_BEST])
    mode = FILL_METHODS[fill_statement.check_method(method)]
    passes = fill_statement.check_passes(passes)
    if plan.n_a != plan.n_b:
        raise ValueError(f'a fill needs the neighbour plan of one grid, and '
                         f'a ({plan.n_b}, {plan.n_a}) plan is not square')
    n = plan.n_b
    if not isinstance(field, torch.Tensor):
        raise TypeError('field must be a tensor (pyremap_amd.fill has the '
                        'numpy twin)')
    field = field.detach()
    if field.device != plan.device:
        raise ValueError('the field and the plan must live on the same '
                         'device')
    shape = [int(s) for s in field.shape]
    axes = [int(ax) + len(shape) if int(ax) < 0 else int(ax) for ax in axes]
    if not axes or len(set(axes)) != len(axes) or \
            any(ax < 0 or ax >= len(shape) for ax in axes):
        raise ValueError(f'axes {axes} are no distinct axes of a field of '
                         f'shape {tuple(shape)}')
    cells = 1
    for ax in axes:
        cells *= shape[ax]
    if cells != n:
        raise ValueError(f'the axes {axes} of a field of shape '
                         f'{tuple(shape)} hold {cells} cells, the grid of the '
                         f'neighbour plan {n}')
    if field.dtype not in (torch.float64, torch.float32):
        field = field.to(torch.float64)
    direct = axes == list(range(axes[0], axes[0] + len(axes)))
    if direct:
        X = field.contiguous()
        B = 1
        for s in shape[:axes[0]]:
            B *= s
        k = 1
        for s in shape[axes[-1] + 1:]:
            k *= s
        back = None
    else:
        others = [ax for ax in range(len(shape)) if ax not in axes]
        order = axes + others
        X = field.permute(order).contiguous()
        B, k = 1, X.numel() // n if n else 0
        back = (list(X.shape), [order.index(ax) for ax in range(len(shape))])
    if info is not None:
        info['passes'] = 0
    out = None
    if X.numel() and (passes is None or passes > 0):
        strides = dict(n_batch=B, k_inner=k, x_row_stride=k,
                       x_batch_stride=n * k, y_row_stride=k,
                       y_batch_stride=n * k, mode=mode, threshold=threshold)
        flat = X.reshape(-1)
        bufs = [torch.empty(flat.numel(), dtype=torch.float64,
                            device=plan.device) for _ in
                range(1 if passes == 1 else 2)]
        mask = torch.empty(flat.numel(), dtype=torch.uint8,
                           device=plan.device) if passes is None else None
        cur, done = flat, 0
        while passes is None or done < passes:
            group = FILL_CHECK_EVERY if passes is None else passes - done
            counts = []
            for g in range(group):
                nxt = bufs[done % len(bufs)]
                apply_strided(plan, cur, nxt, mask_out=mask, **strides)
                cur, done = nxt, done + 1
                if mask is not None and g >= group - 2:
                    counts.append(mask.sum(dtype=torch.int64))
            if passes is not None:
                break
            before, after = (int(c) for c in torch.stack(counts).cpu())
            if after == 0 or after == before:
                if info is not None:
                    info['missing'] = after
                break
        out = cur
        if info is not None:
            info['passes'] = done
    if out is None:
        out = X.to(torch.float64).reshape(-1)
        if out.data_ptr() == field.data_ptr():
            out = out.clone()
        if info is not None and passes is None:
            info['missing'] = int(torch.isnan(out).sum())
    out = out.reshape(X.shape)
    if back is not None:
        out = out.permute(back[1]).contiguous()
    return out.reshape(shape)


def _sgs_group(frac, shape, axes):
    """How the axes ``axes`` of ``frac`` stand against a field of ``shape``:
    ``(frac, full)`` -- ``full`` if every one has the field's extent, not
    ``full`` if every one has extent 1; a group that mixes the two is
    expanded to the field's extents first (one device copy later, when the
    fraction is made contiguous)."""
    full = all(int(frac.shape[ax]) == int(shape[ax]) for ax in axes)
    if full or all(int(frac.shape[ax]) == 1 for ax in axes):
        return frac, full
    sizes = [int(shape[ax]) if ax in axes else -1
             for ax in range(frac.ndim)]
    return frac.expand(sizes), True


def remap_tensor_sgs(plan, dst_grid_dims, field, frac, remap_axes,
                     threshold=0.0):
    """
    :func:`remap_tensor` with sub-gridscale fraction weighting
    (:mod:`pyremap_amd.sgs`; NCO's ``ncremap --sgs_frc``): ``field`` is a
    mean over the fraction ``frac`` of every source cell; the result is
    ``A.(frac * field) / A.frac`` with NaN in either skipped, in ONE launch
    (``remap_apply_sgs``).  Same result shape and axis order as
    :func:`remap_tensor`, NaN where ``valid <= threshold`` or the remapped
    fraction is not positive.

    ``frac`` has ``field``'s number of axes, its remap axes at full extent and
    every other axis at the field's extent or 1.  Leading and trailing axis
    groups that are uniformly full or uniformly 1 become strides (a stride of
    0 broadcasts); a group that mixes the two is expanded once on the device.
    One device only.
    """
    torch = _torch()
    _one_device(plan, 'sub-gridscale weighting')
    remap_axes, dst_shape = check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_grid_dims, field.shape,
        remap_axes)
    ndim = field.ndim
    if frac.ndim != ndim:
        raise ValueError(f'frac has {frac.ndim} axes, the field {ndim}')
    if frac.device != field.device:
        raise ValueError('frac and the field must live on the same device')
    for ax in range(ndim):
        want = int(field.shape[ax])
        if int(frac.shape[ax]) != want and \
                (ax in remap_axes or int(frac.shape[ax]) != 1):
            raise ValueError(
                f'frac of shape {tuple(frac.shape)} against a field of shape '
                f'{tuple(field.shape)}: axis {ax} must have extent {want}' +
                ('' if ax in remap_axes else ' or 1'))
    if field.dtype not in (torch.float64, torch.float32):
        field = field.to(torch.float64)
    if frac.dtype not in (torch.float64, torch.float32):
        frac = frac.to(torch.float64)
    lay = field_layout(plan, field.shape, remap_axes, dst_shape)
    # the fraction's strides: every group of axes is there in full, or is
    # broadcast (a stride of 0)
    frac, lead_full = _sgs_group(frac, field.shape, lay.groups[0])
    frac, mid_full = _sgs_group(frac, field.shape, lay.groups[1])
    frac, tail_full = _sgs_group(frac, field.shape, lay.groups[2])
    k_inner = lay.strides['k_inner']
    kf = k_inner if tail_full else 1
    f_strides = dict(f_row_stride=kf, f_batch_stride=0,
                     f_inner_stride=1 if tail_full else 0)
    f_launches = 1
    if lay.route == 'direct' and lead_full:
        f_strides['f_batch_stride'] = plan.n_a * kf
    elif lay.route == 'fold':
        nx = lay.strides['x_src_fold']
        if mid_full:
            f_strides['f_batch_stride'] = nx * kf
        f_strides['f_outer_stride'] = \
            (lay.strides['n_batch'] if mid_full else 1) * nx * kf
        f_launches = lay.n_launch if lead_full else 1
    X = _launch_source(plan, lay, field, k_inner)
    F = _launch_source(plan, lay, frac, kf)
    Y = torch.empty(lay.y_shape, dtype=torch.float64, device=field.device)
    Fs = [Fl for Fl, in _launch_rows(f_launches, F)]
    for li, (Xl, Yl) in enumerate(_launch_rows(lay.n_launch, X, Y)):
        sgs_strided(plan, Xl, Fs[li if f_launches > 1 else 0], Yl,
                    threshold=threshold, **f_strides, **lay.strides)
    return _launch_result(lay, Y)


def _asked_for(torch, values, name, device, shape_ok, expected):
    """What a column pass is asked for (``name``: the targets, the bounds) as
    a contiguous float64 tensor on ``device``, of a shape that ``shape_ok``
    accepts (``expected`` in words)."""
    if isinstance(values, torch.Tensor):
        if values.device != device:
            raise ValueError(f'{name} and the field must live on the same '
                             f'device')
        if not (values.dtype.is_floating_point or
                values.dtype in (torch.int32, torch.int64)):
            raise ValueError(f'{name} of dtype {values.dtype}: expected '
                             f'numbers')
        Q = values.to(torch.float64)
    else:
        Q = torch.as_tensor(values, dtype=torch.float64).to(device)
    if not shape_ok(Q):
        raise ValueError(f'{name} of shape {tuple(Q.shape)}: expected a '
                         f'non-empty {expected}')
    return Q.contiguous()


def remap_tensor_levels(plan, dst_grid_dims, field, z, targets, remap_axes,
                        threshold=0.0):
    """
    :func:`remap_tensor` of a field interpolated to target levels
    (:mod:`pyremap_amd.levels`; depth slices): the LAST axis of ``field`` is
    its level axis, ``z`` the coordinate of every level (``zMid``),
    ``targets`` the ``L`` levels asked for, in any order.  Every entry of a
    row interpolates its source column to the target level first -- linear
    between the two levels that bracket it, no value where none do, nothing
    extrapolated -- and enters the masked, renormalised sum then, in ONE
    launch per :func:`field_layout` launch (``remap_apply_levels``).  The
    result has the shape and axis order of :func:`remap_tensor` with ``L`` in
    place of ``n_levels``; float64, NaN where ``valid <= threshold``.

    ``z`` has ``field``'s number of axes, the level axis at full extent, the
    remap axes at full extent or all 1 (one coordinate for all cells) and
    every other axis at the field's extent or 1 (a time-invariant
    coordinate).  Groups of axes that are uniformly full or uniformly 1
    become strides (a stride of 0 broadcasts); a group that mixes the two is
    expanded once on the device.  One device only.
    """
    _one_device(plan, 'the level interpolation')

    def launch(X, Z, T, Y, *, c_row_stride, c_batch_stride, c_outer_stride=0,
               **strides):
        levels_strided(plan, X, Z, T, Y, threshold=threshold,
                       z_row_stride=c_row_stride,
                       z_batch_stride=c_batch_stride,
                       z_outer_stride=c_outer_stride, **strides)

    def outputs(torch, device):
        T = _asked_for(torch, targets, 'targets', device,
                       lambda T: T.ndim == 1 and T.numel() > 0,
                       '1-D list of levels')
        return T, int(T.numel())
    return _remap_tensor_columns(plan, dst_grid_dims, field, z, 'z',
                                 remap_axes, outputs, launch)


def _reduce_code(reduce):
    if reduce not in REDUCE:
        raise ValueError(f'reduce {reduce!r}: expected one of '
                         f'{sorted(REDUCE)}')
    return REDUCE[reduce]


def remap_tensor_layers(plan, dst_grid_dims, field, thickness, bounds,
                        remap_axes, threshold=0.0, reduce='mean'):
    """
    :func:`remap_tensor` of a field averaged (``reduce='mean'``) or
    integrated (``'integral'``) over depth ranges (:mod:`pyremap_amd.layers`;
    layer means, heat content): the LAST axis of ``field`` is its level axis,
    ``thickness`` the thickness of every layer (``layerThickness``),
    ``bounds`` the ``R`` ranges ``(A, B)`` asked for, depths positive
    downward from the top of each column, in any order, ``B = inf`` "to the
    bottom".  Every entry of a row reduces its source column over the range
    first -- every layer weighted by its overlap with the range, a column
    that ends above the range skipped as a NaN is -- and enters the masked,
    renormalised sum then, in ONE launch per :func:`field_layout` launch
    (``remap_apply_layers``).  The result has the shape and axis order of
    :func:`remap_tensor` with ``R`` in place of ``n_levels``; float64, NaN
    where ``valid <= threshold``.

    ``thickness`` broadcasts as ``z`` of :func:`remap_tensor_levels` does:
    the level axis at full extent, the remap axes at full extent or all 1,
    every other axis at the field's extent or 1 (a time-invariant thickness),
    through strides of 0.  One device only.
    """
    _one_device(plan, 'the layer reduction')
    _reduce_code(reduce)

    def launch(X, H, Bd, Y, *, c_row_stride, c_batch_stride, c_outer_stride=0,
               **strides):
        layers_strided(plan, X, H, Bd, Y, threshold=threshold, reduce=reduce,
                       h_row_stride=c_row_stride,
                       h_batch_stride=c_batch_stride,
                       h_outer_stride=c_outer_stride, **strides)

    def outputs(torch, device):
        Bd = _asked_for(torch, bounds, 'bounds', device,
                        lambda Bd: Bd.ndim == 2 and Bd.shape[1] == 2 and
                        Bd.shape[0] > 0, 'list of (top, bottom) pairs')
        return Bd, int(Bd.shape[0])
    return _remap_tensor_columns(plan, dst_grid_dims, field, thickness,
                                 'thickness', remap_axes, outputs, launch)


def _remap_tensor_columns(plan, dst_grid_dims, field, z, zname, remap_axes,
                          outputs, launch):
    """
    What :func:`remap_tensor_levels` and :func:`remap_tensor_layers` share: a
    field whose LAST axis is its level axis, reduced column by column inside
    the apply with a companion ``z`` (called ``zname`` in messages: the level
    coordinate, the layer thicknesses) that broadcasts over the field.  The
    checks, the routes and strides of :func:`field_layout` and the launches.
    ``outputs(torch, device)``: the float64 device tensor of what is asked
    for (targets; ranges) and the inner extent of the result (their number);
    ``launch(X, Z, T, Y, **strides)``: one launch, the companion's strides
    under the names ``c_row_stride``, ``c_batch_stride``, ``c_outer_stride``.
    """
    torch = _torch()
    ndim = field.ndim
    for name, t in (('field', field), (zname, z)):
        if not isinstance(t, torch.Tensor):
            raise ValueError(f'{name} must be a device tensor')
        if not t.dtype.is_floating_point:
            raise ValueError(f'{name} of dtype {t.dtype}: expected a '
                             f'floating dtype')
    if ndim < 2:
        raise ValueError('the field needs a level axis behind its remap axes')
    remap_axes, dst_shape = check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_grid_dims, field.shape,
        remap_axes)
    if ndim - 1 in remap_axes:
        raise ValueError('the last axis of the field is its level axis: it '
                         'cannot be a remap axis')
    if z.ndim != ndim:
        raise ValueError(f'{zname} has {z.ndim} axes, the field {ndim}')
    if z.device != field.device:
        raise ValueError(f'{zname} and the field must live on the same '
                         f'device')
    shape = [int(s) for s in field.shape]
    n_levels = shape[-1]
    if n_levels < 1:
        raise ValueError('the level axis is empty')
    z_cells = [int(z.shape[ax]) == shape[ax] for ax in remap_axes]
    for ax in range(ndim):
        have, want = int(z.shape[ax]), shape[ax]
        full_only = ax == ndim - 1
        if have != want and (full_only or have != 1):
            raise ValueError(
                f'{zname} of shape {tuple(z.shape)} against a field of shape '
                f'{tuple(field.shape)}: axis {ax} must have extent {want}' +
                ('' if full_only else ' or 1'))
    if not all(z_cells) and any(int(z.shape[ax]) != 1 for ax in remap_axes):
        raise ValueError(
            f'{zname} of shape {tuple(z.shape)}: the remap axes {remap_axes} '
            f'must all have the field\'s extent or all have extent 1')
    z_cells = all(z_cells)
    T, L = outputs(torch, field.device)
    if field.dtype not in (torch.float64, torch.float32):
        field = field.to(torch.float64)
    if z.dtype not in (torch.float64, torch.float32):
        z = z.to(torch.float64)
    lay = field_layout(plan, shape, remap_axes, dst_shape)
    if lay.route == 'fold' and len(lay.groups[2]) > 1:
        # (dims between the last source axis and the levels: transposed)
        lay = field_layout(plan, shape, remap_axes, dst_shape, fold=False)
    n_a, n_b = plan.n_a, plan.n_b
    n_az = n_a if z_cells else 1
    nl = n_levels
    level_axis = ndim - 1
    if lay.route == 'permute':
        extras = [ax for ax in lay.groups[2] if ax != level_axis]
        z, mid_full = _sgs_group(z, shape, extras)
        M = _prod(shape[ax] for ax in extras)
        Mz = M if mid_full else 1
        X = field.permute(lay.order).reshape(n_a, M * nl).contiguous()
        Z = z.permute(lay.order).reshape(n_az, Mz * nl).contiguous()
        strides = dict(n_batch=M, x_batch_stride=nl, x_row_stride=M * nl,
                       y_batch_stride=L, y_row_stride=M * L,
                       c_batch_stride=nl if mid_full else 0,
                       c_row_stride=Mz * nl if z_cells else 0)
        n_launch, lead_full = 1, False
        y_shape = [n_b, M * L]
        back_shape, unpermute = lay.back
        back = (list(back_shape[:-1]) + [L], unpermute)
    elif lay.route == 'fold':
        lead, mid = list(lay.groups[0]), list(lay.groups[1])
        z, lead_full = _sgs_group(z, shape, lead)
        z, mid_full = _sgs_group(z, shape, mid)
        nx = lay.strides['x_src_fold']
        M = lay.strides['n_batch']
        Mz = M if mid_full else 1
        X, Z = field.contiguous(), z.contiguous()
        strides = dict(n_batch=M, x_row_stride=nl, x_batch_stride=nx * nl,
                       x_src_fold=nx, x_outer_stride=M * nx * nl,
                       y_row_stride=M * L, y_batch_stride=L)
        if z_cells:
            strides.update(c_row_stride=nl, c_outer_stride=Mz * nx * nl,
                           c_batch_stride=nx * nl if mid_full else 0)
        else:
            strides.update(c_row_stride=0, c_outer_stride=0,
                           c_batch_stride=nl if mid_full else 0)
        n_launch = lay.n_launch
        y_shape, back = list(lay.out_shape[:-1]) + [L], None
    else:
        lead = list(lay.groups[0])
        mid = [ax for ax in lay.groups[2] if ax != level_axis]
        z, lead_full = _sgs_group(z, shape, lead)
        z, mid_full = _sgs_group(z, shape, mid)
        NB = _prod(shape[ax] for ax in lead)
        M = _prod(shape[ax] for ax in mid)
        Mz = M if mid_full else 1
        X, Z = field.contiguous(), z.contiguous()
        if M == 1:
            # (Time, nCells, nVertLevels): the dims in front are the batches
            strides = dict(n_batch=NB, x_row_stride=nl,
                           x_batch_stride=n_a * nl, y_row_stride=L,
                           y_batch_stride=n_b * L,
                           c_row_stride=nl if z_cells else 0,
                           c_batch_stride=n_az * nl if lead_full else 0)
            n_launch, lead_full = 1, False
        else:
            # dims between the source axes and the levels are the batches,
            # one launch per index of the dims in front
            strides = dict(n_batch=M, x_batch_stride=nl, x_row_stride=M * nl,
                           y_batch_stride=L, y_row_stride=M * L,
                           c_batch_stride=nl if mid_full else 0,
                           c_row_stride=Mz * nl if z_cells else 0)
            n_launch = NB
        y_shape, back = list(lay.out_shape[:-1]) + [L], None
    Y = torch.empty(y_shape, dtype=torch.float64, device=field.device)
    Zs = [Zl for Zl, in _launch_rows(n_launch if lead_full else 1, Z)]
    for li, (Xl, Yl) in enumerate(_launch_rows(n_launch, X, Y)):
        launch(Xl, Zs[li if lead_full else 0], T, Yl, **strides,
               n_levels=nl, k_inner=L)
    if back is None:
        return Y
    return Y.reshape(back[0]).permute(back[1]).contiguous()


def remap_tensor_vector(plan, dst_grid_dims, u, v, basis_a, basis_b,
                        remap_axes, threshold=0.0):
    """
    :func:`remap_tensor` for the eastward and northward components ``u`` and
    ``v`` of a vector field (:mod:`pyremap_amd.vector`): every source vector
    is rotated to Cartesian with ``basis_a (n_a, 5)``, the rows' weighted sums
    are projected on ``basis_b (n_b, 5)``, NaN in either component is
    skipped, all in ONE launch per :func:`field_layout` launch
    (``remap_apply_vector``).  Returns ``(yu, yv)``, each with the result
    shape and axis order of :func:`remap_tensor`, NaN where ``valid <=
    threshold``.  ``u`` and ``v`` have one shape, dtype and device; nothing
    is copied where a field is addressable in place.  One device only.
    """
    torch = _torch()
    _one_device(plan, 'the vector remap')
    if tuple(u.shape) != tuple(v.shape) or u.dtype != v.dtype:
        raise ValueError(
            f'u of shape {tuple(u.shape)} and dtype {u.dtype}, v of shape '
            f'{tuple(v.shape)} and dtype {v.dtype}: expected one shape and '
            f'one dtype')
    if u.device != v.device:
        raise ValueError('u and v must live on the same device')
    remap_axes, dst_shape = check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_grid_dims, u.shape,
        remap_axes)
    if u.dtype not in (torch.float64, torch.float32):
        u, v = u.to(torch.float64), v.to(torch.float64)
    lay = field_layout(plan, u.shape, remap_axes, dst_shape)
    k_inner = lay.strides['k_inner']
    U = _launch_source(plan, lay, u, k_inner)
    V = _launch_source(plan, lay, v, k_inner)
    YU = torch.empty(lay.y_shape, dtype=torch.float64, device=u.device)
    YV = torch.empty(lay.y_shape, dtype=torch.float64, device=u.device)
    for Ul, Vl, YUl, YVl in _launch_rows(lay.n_launch, U, V, YU, YV):
        vector_strided(plan, Ul, Vl, basis_a, basis_b, YUl, YVl,
                       threshold=threshold, **lay.strides)
    return _launch_result(lay, YU), _launch_result(lay, YV)


def scan_nan(x, flag):
    """
    Asynchronously OR 1 into ``flag`` (int32 device tensor, zeroed by the
    caller) if the float32/float64 device tensor ``x`` holds a NaN: the
    device half of ``remap_numpy.py:201-204``.  A ``flag`` of two elements
    also receives the KIND of the missing values (``remap_scan_nan_kinds``):
    ``flag[1]`` = 0 (no NaN), 1 (NaNs in whole aligned runs: whole cells of
    an ``(n_a, K)`` field) or 3 (NaNs column by column).
    """
    torch = _torch()
    lib = load_library()
    if not x.is_contiguous():
        raise ValueError('scan_nan needs a contiguous tensor')
    dtype = {torch.float64: DTYPE_F64, torch.float32: DTYPE_F32}[x.dtype]
    fn, name = (lib.remap_scan_nan_kinds, 'remap_scan_nan_kinds') \
        if flag.numel() >= 2 else (lib.remap_scan_nan, 'remap_scan_nan')
    with torch.cuda.device(x.device):
        _check(fn(_ptr(x), dtype, x.numel(), _ptr(flag),
                  _stream_ptr(x.device)), name)


def scan_nan_layout(x, n_rows, n_batch, k_inner, kinds):
    """
    The NaN scan with the field's layout (``remap_scan_nan_layout``): ``x`` a
    contiguous device tensor holding ``n_batch`` batches of ``n_rows`` source
    cells of ``k_inner`` contiguous values -- ``(Time, nCells, nVertLevels)``
    -- and ``kinds`` four zeroed int32: any NaN; whole cells missing (1) or
    not (3); the same mask in every batch (1) or not (3); the masked form that
    suits (0 none, 1 ``FLAG_CELL_MASKS``, 2 ``FLAG_BATCH_MASKS``, 3 neither).
    """
    torch = _torch()
    lib = load_library()
    if not x.is_contiguous() or x.numel() != n_batch * n_rows * k_inner:
        raise ValueError('scan_nan_layout needs a contiguous (n_batch, '
                         'n_rows, k_inner) tensor')
    if kinds.numel() < 4 or kinds.dtype != torch.int32:
        raise ValueError('kinds: four int32')
    dtype = {torch.float64: DTYPE_F64, torch.float32: DTYPE_F32}[x.dtype]
    with torch.cuda.device(x.device):
        _check(lib.remap_scan_nan_layout(
            _ptr(x), dtype, n_rows, n_batch, k_inner, k_inner,
            n_rows * k_inner, _ptr(kinds), _stream_ptr(x.device)),
            'remap_scan_nan_layout')


def cell_mask_form(plan):
    """Does ``plan`` run the masked mode faster with FLAG_CELL_MASKS when
    whole cells are missing (8-row groups: entry-rich mappings)?"""
    groups = getattr(plan, 'groups', None)
    return bool(groups) and groups.get('rows') == 8


def remap_tensor_auto_mode(plan, dst_grid_dims, field, remap_axes, threshold,
                           flags=0, out=None, flag=None, limiter=None,
                           row_weight=None):
    """
    ``_remap_data_array``'s branch (``remap_numpy.py:201-204``) without a
    host round trip: the masked, renormalised result if ``field`` holds a
    NaN, the ``frac_b``-normalised one if not.  One scan, two gated launches
    (the one whose gate is closed does nothing; three on entry-rich mappings,
    whose masked branch has two forms), nothing synchronises.  ``limiter`` /
    ``row_weight`` as in :func:`remap_tensor`: the limiter runs ONCE behind
    the gated launches, ungated -- it sees ``Y`` as whichever of them left it
    and needs no mode.
    """
    torch = _torch()
    weight = _limiter_arguments(plan, limiter, row_weight)
    # (before the scan below is enqueued: remap_tensor would say the same,
    # but only after it)
    axes, dst_shape = check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_grid_dims, field.shape,
        remap_axes)
    if hasattr(plan, 'shards'):
        if out is not None or flag is not None:
            raise ValueError("out / flag address ONE device's launch; not "
                             'with a multi-device plan')
        return plan.remap_tensor_auto_mode(dst_grid_dims, field, remap_axes,
                                           threshold, flags=flags)
    if not in_place_addressable(field.shape, remap_axes):
        # permute copies either side of the launch: decide with one readback
        masked = bool(torch.isnan(field).any())
        return remap_tensor(plan, dst_grid_dims, field, remap_axes,
                            MODE_MASKED if masked else MODE_FRACB,
                            threshold=threshold if masked else 0.0,
                            flags=flags, out=out, limiter=limiter,
                            row_weight=weight)
    X = field.contiguous()
    lay = field_layout(plan, X.shape, axes, dst_shape)    # ('direct')

    def limited(Y):
        if limiter is not None:
            _limit_after_apply(plan, limiter, weight, X, Y, **lay.strides)
        return Y
    if flag is None and cell_mask_form(plan):
        # entry-rich mapping: the scan -- told where the cells and the
        # batches of the field are -- also says whether whole cells are
        # missing (land) or the mask is the same in every batch
        # (bathymetry), and the masked branch comes in the form that suits
        # (REMAP_FLAG_CELL_MASKS / REMAP_FLAG_BATCH_MASKS / neither): up to
        # four gated launches, one of which runs
        n_batch, k_inner = lay.strides['n_batch'], lay.strides['k_inner']
        hints = FLAG_CELL_MASKS | FLAG_BATCH_MASKS
        flags &= ~hints
        kinds = torch.zeros(4, dtype=torch.int32, device=field.device)
        scan_nan_layout(X, plan.n_a, n_batch, k_inner, kinds)
        Y = remap_tensor(plan, dst_grid_dims, X, remap_axes, MODE_MASKED,
                         threshold=threshold, flags=flags | FLAG_CELL_MASKS,
                         out=out, gate=kinds[3:], gate_value=1)
        if n_batch >= 3:
            Y = remap_tensor(plan, dst_grid_dims, X, remap_axes, MODE_MASKED,
                             threshold=threshold,
                             flags=flags | FLAG_BATCH_MASKS, out=Y,
                             gate=kinds[3:], gate_value=2)
        Y = remap_tensor(plan, dst_grid_dims, X, remap_axes, MODE_MASKED,
                         threshold=threshold, flags=flags, out=Y,
                         gate=kinds[3:], gate_value=3)
        return limited(remap_tensor(
            plan, dst_grid_dims, X, remap_axes, MODE_FRACB, flags=flags,
            out=Y, gate=kinds, gate_value=0))
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=field.device)
    scan_nan(X, flag)
    Y = remap_tensor(plan, dst_grid_dims, X, remap_axes, MODE_MASKED,
                     threshold=threshold, flags=flags, out=out, gate=flag,
                     gate_value=1)
    return limited(remap_tensor(
        plan, dst_grid_dims, X, remap_axes, MODE_FRACB, flags=flags, out=Y,
        gate=flag, gate_value=0))


def _adjoint_field_shape(cot_shape, remap_axes, src_grid_dims, n_dst):
    """The shape of the field whose result has ``cot_shape``: the source dims
    at ``remap_axes``, the result's other dims, in their order, elsewhere."""
    src = [int(d) for d in src_grid_dims]
    if len(src) != len(remap_axes):
        raise ValueError(f'src_grid_dims {src} and remap_axes '
                         f'{list(remap_axes)} differ in length')
    ndim = len(cot_shape) - n_dst + len(src)
    if ndim < len(src):
        raise ValueError(f'a cotangent of shape {tuple(cot_shape)} is no '
                         f'result on {n_dst} destination dims')
    axes = [int(a) % ndim for a in remap_axes]
    lead = min(axes)
    extras = iter(list(cot_shape[:lead]) + list(cot_shape[lead + n_dst:]))
    return [src[axes.index(ax)] if ax in axes else int(next(extras))
            for ax in range(ndim)]


def _argsort(perm):
    return sorted(range(len(perm)), key=perm.__getitem__)


def _adjoint(plan, src_grid_dims, cotangent, remap_axes, field, passes,
             dst_grid_dims, fill):
    """What :func:`remap_tensor_adjoint` and its auto mode share.  ``passes``:
    the cotangent launches as ``(mode, threshold, gate, gate_value)``."""
    torch = _torch()
    G = cotangent
    if G.device != plan.device or (field is not None and
                                   field.device != plan.device):
        raise ValueError('the cotangent, the field and the plan must live on '
                         'the same device')
    if not G.dtype.is_floating_point:
        raise TypeError(f'the cotangent must be floating point, not '
                        f'{G.dtype}')
    dst_shape = [plan.n_b] if dst_grid_dims is None else \
        [int(d) for d in dst_grid_dims]
    if field is not None:
        shape = [int(s) for s in field.shape]
        if field.dtype not in (torch.float64, torch.float32):
            field = field.to(torch.float64)     # (as the forward read it)
    else:
        shape = _adjoint_field_shape(G.shape, remap_axes, src_grid_dims,
                                     len(dst_shape))
    axes, dst_shape = check_field_extents(
        plan.n_a, plan.n_b, plan.n_b_global, dst_shape, shape, remap_axes)
    if field is not None and src_grid_dims is not None and \
            _prod(src_grid_dims) != plan.n_a:
        raise ValueError(f'src_grid_dims {list(src_grid_dims)} do not hold '
                         f'n_a = {plan.n_a} cells')
    gated = any(p[2] is not None for p in passes)
    lay = field_layout(plan, shape, axes, dst_shape, fold=not gated)
    if tuple(G.shape) != tuple(lay.out_shape):
        raise ValueError(
            f'the cotangent has shape {tuple(G.shape)}; the result of a '
            f'field of shape {tuple(shape)} has {tuple(lay.out_shape)}')
    if gated and lay.route != 'direct':
        raise ValueError('gated launches need the source axes adjacent '
                         '(in-place addressing)')
    tplan = plan.transposed()
    # 1. G into the buffer the forward's launches wrote, float64
    T = torch.empty(lay.y_shape, dtype=torch.float64, device=plan.device)
    if lay.back is None:
        T.copy_(G)
    else:
        back_shape, unpermute = lay.back
        T.view(back_shape).copy_(G.permute(_argsort(unpermute)))
    # 2. the cotangent of the division, in place, with the forward's strides
    needs_x = any(p[0] == MODE_COTAN_MASKED for p in passes)
    X = _launch_source(plan, lay, field, lay.strides['k_inner']) \
        if needs_x else None
    for Xl, Tl in _launch_rows(lay.n_launch, X, T):
        for mode, threshold, gate, gate_value in passes:
            cotangent_strided(plan, Xl, Tl, mode=mode, threshold=threshold,
                              gate=gate, gate_value=gate_value, **lay.strides)
    # 3. the transposed sum: MODE_RAW with S^T over the one axis of rows
    if lay.route == 'direct':
        lead = [shape[ax] for ax in lay.groups[0]]
        tail = [shape[ax] for ax in lay.groups[2]]
        Tv, axis = T.view(lead + [plan.n_b] + tail), len(lead)
    elif lay.route == 'fold':
        Tv, axis = T.view(lay.n_launch, plan.n_b, -1), 1
    else:
        Tv, axis = T, 0
    gX = remap_tensor(tplan, None, Tv, [axis], MODE_RAW, flags=0)
    # 4. into the field's shape
    if lay.route == 'fold':
        a0, a1 = axes
        ny, nx = shape[a0], shape[a1]
        M, Tt = lay.strides['n_batch'], lay.strides['k_inner']
        gX = gX.view(lay.n_launch, ny, nx, M, Tt).permute(0, 1, 3, 2, 4)
    elif lay.route == 'permute':
        gX = gX.view([shape[ax] for ax in lay.order]).permute(
            _argsort(lay.order))
    gX = gX.reshape(shape).contiguous()
    # 5. missing sources take nothing
    if fill:
        gX.masked_fill_(torch.isnan(field), 0.0)
    return gX


_COTAN_OF = {MODE_FRACB: MODE_COTAN_FRACB, MODE_MASKED: MODE_COTAN_MASKED}


def remap_tensor_adjoint(plan, src_grid_dims, cotangent, remap_axes, mode,
                         field=None, threshold=0.0, gate=None, gate_value=0,
                         dst_grid_dims=None):
    """
    The adjoint of :func:`remap_tensor` in ``mode`` (``MODE_RAW``,
    ``MODE_FRACB`` or ``MODE_MASKED``): ``gX = dL/dfield`` for the cotangent
    ``dL/dy`` of its result, a float64 device tensor of the field's shape
    (:mod:`pyremap_amd.adjoint` has the definition to the bit).

    ``cotangent`` has the shape of the forward's result; ``remap_axes`` are
    the forward's, the axes of the FIELD that hold the source grid, in place,
    folded or permuted as the forward accepts them.  ``field`` is the
    forward's field: required behind ``MODE_MASKED`` (read for NaN only),
    else optional -- without it ``src_grid_dims`` (C order) says what
    ``remap_axes`` hold.  ``dst_grid_dims``: the destination dims of the
    forward (``None``: flat rows).

    The cotangent is copied into a float64 buffer, divided in place by one
    launch of ``csrc/apply_cotangent.h`` with the forward's own strides
    (``gate`` / ``gate_value`` gate it, in-place layouts only; ``MODE_RAW``:
    no launch), summed by ``remap_tensor(plan.transposed(), ..., MODE_RAW,
    flags=0)`` and brought into the field's shape; behind ``MODE_MASKED``
    ``+0.0`` is filled in where the field is NaN.  The first call builds
    ``plan.transposed()``.  One device; no limiter has an adjoint.
    """
    _one_device(plan, 'the adjoint apply')
    if mode not in (MODE_RAW, MODE_FRACB, MODE_MASKED):
        raise ValueError(f'the adjoint apply serves MODE_RAW, MODE_FRACB and '
                         f'MODE_MASKED, not mode {mode}')
    if mode == MODE_MASKED and field is None:
        raise ValueError("the adjoint of the masked mode needs the forward's "
                         'field: its NaNs say what the forward divided by')
    if field is None and src_grid_dims is None:
        raise ValueError('give the field or src_grid_dims')
    passes = [] if mode == MODE_RAW else \
        [(_COTAN_OF[mode], threshold, gate, gate_value)]
    return _adjoint(plan, src_grid_dims, cotangent, remap_axes, field, passes,
                    dst_grid_dims, fill=mode == MODE_MASKED)


def remap_tensor_adjoint_auto_mode(plan, src_grid_dims, cotangent, remap_axes,
                                   field, threshold, dst_grid_dims=None,
                                   flag=None):
    """
    The adjoint of :func:`remap_tensor_auto_mode`, with its branch and, like
    it, without a host round trip: one scan of ``field`` into a flag, the
    masked cotangent gated on a NaN found, the ``frac_b`` one on none, one
    transposed sum, the fill.  A field whose source axes are not adjacent
    decides with one readback, as the forward does.
    """
    torch = _torch()
    _one_device(plan, 'the adjoint apply')
    if field is None:
        raise ValueError("the adjoint of the auto mode needs the forward's "
                         'field')
    if field.dtype not in (torch.float64, torch.float32):
        field = field.to(torch.float64)
    if not in_place_addressable(field.shape, remap_axes):
        masked = bool(torch.isnan(field).any())
        return remap_tensor_adjoint(
            plan, src_grid_dims, cotangent, remap_axes,
            MODE_MASKED if masked else MODE_FRACB, field=field,
            threshold=threshold if masked else 0.0,
            dst_grid_dims=dst_grid_dims)
    X = field.contiguous()
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=field.device)
    scan_nan(X, flag)
    passes = [(MODE_COTAN_MASKED, threshold, flag, 1),
              (MODE_COTAN_FRACB, 0.0, flag, 0)]
    return _adjoint(plan, src_grid_dims, cotangent, remap_axes, X, passes,
                    dst_grid_dims, fill=True)


def gather_rows(field, axis, rows, out=None):
    """
    ``field.index_select(axis, rows)`` for a contiguous device tensor through
    the library's ``remap_gather_rows``: the packed source buffer
    ``X[ucols]`` a row shard's GPU receives.  ``rows``: int32 device tensor.
    Asynchronous on torch's current stream.

    Every listed row must lie below ``field.shape[axis]``: the kernel reads
    ``field`` at each of them and has no bound, and reading ``rows`` back to
    compare would synchronise the stream.  The callers check the field's
    extent against the mapping the rows come from
    (:func:`check_field_extents`) before they get here.
    """
    torch = _torch()
    lib = load_library()
    if not field.is_contiguous():
        field = field.contiguous()
    axis = int(axis) % field.ndim
    if rows.dtype != torch.int32 or rows.device != field.device:
        rows = rows.to(device=field.device, dtype=torch.int32)
    rows = rows.contiguous()
    n_batch = _prod(field.shape[:axis])
    inner = _prod(field.shape[axis + 1:])
    item = field.element_size()
    shape = list(field.shape[:axis]) + [int(rows.shape[0])] + \
        list(field.shape[axis + 1:])
    if out is None:
        out = torch.empty(shape, dtype=field.dtype, device=field.device)
    elif list(out.shape) != shape or out.dtype != field.dtype or \
            out.device != field.device or not out.is_contiguous():
        raise ValueError(f'out must be a contiguous {field.dtype} tensor of '
                         f'shape {tuple(shape)} on {field.device}')
    with torch.cuda.device(field.device):
        _check(lib.remap_gather_rows(
            _ptr(field), n_batch, int(field.shape[axis]) * inner * item,
            inner * item, _ptr(rows), int(rows.shape[0]), inner * item,
            _ptr(out), _stream_ptr(field.device)), 'remap_gather_rows')
    return out


def clock_probe(device, micros=20):
    """
    Enqueue a shader-clock measurement on torch's current stream of
    ``device`` (``remap_clock_probe``: one wave spinning for ``micros`` us).
    Returns a function that, once the stream has been synchronised, gives
    the clock in MHz the chip held at that point of the stream.
    """
    torch = _torch()
    lib = load_library()
    device = torch.device(device)
    ticks = torch.zeros(2, dtype=torch.int64, device=device)
    with torch.cuda.device(device):
        _check(lib.remap_clock_probe(_ptr(ticks), int(micros),
                                     _stream_ptr(device)),
               'remap_clock_probe')

    def mhz():
        t, r = (int(v) for v in ticks.cpu())
        return 100.0 * t / r if r else float('nan')
    return mhz


def stream_copy(dst, src):
    """Asynchronous device copy through the library's streaming kernel."""
    torch = _torch()
    lib = load_library()
    nbytes = src.numel() * src.element_size()
    with torch.cuda.device(src.device):
        _check(lib.remap_stream_copy(_ptr(dst), _ptr(src), nbytes,
                                     _stream_ptr(src.device)),
               'remap_stream_copy')


# ---------------------------------------------------------------------------
# weight generation (geometry.py), under the names the package calls it by
# ---------------------------------------------------------------------------

from pyremap_amd.geometry import (  # noqa: E402,F401
    CELL_AREAS_MAX_WIDTH, NEAREST_K_MAX, OVERLAP_MAX_EDGES, PATCH_FIT_WIDTH,
    PATCH_MAX_RING, PIECES_PHASES, cell_areas, cell_moments,
    column_fractions, conserve2nd_assemble, expand_cells, gradient_stencils,
    locate_in_quads, locate_in_triangles, nearest_k_points, nearest_points,
    node_rings, overlap_grids, overlap_latlon, overlap_meshes,
    overlap_moments, overlap_pieces, patch_fits, patch_rows)
