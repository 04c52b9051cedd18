"""
The contract between a field and a mapping (`engine.check_field_extents`):
the remapped axes hold exactly `n_a` source cells and `dst_grid_dims` exactly
`n_b`.  Everything behind it addresses raw pointers with those two numbers,
so every route to a launch states it before anything else.

Here, without a GPU: the checker alone, and -- on stand-in plans that own no
device memory -- that each route whose first lines run without a device
raises it BEFORE its first gather, scan or launch (the doors to the raw
pointers are replaced by functions that fail the test).  The routes on a real
device: tests/test_gpu_route_contracts.py.
"""
import types

import numpy as np
import pytest

N_A, N_B = 1500, 2280             # 30 x 50 source cells -> 38 x 60
DST = (38, 60)
SRC_TEXT = r'the remapped axes hold {} source cells but the mapping has ' \
           r'n_a = 1500'
DST_TEXT = r'dst_grid_dims \[{}\] do not hold n_b = 2280 cells'


def _plan(**kw):
    base = dict(n_a=N_A, n_b=N_B, n_b_global=N_B)
    base.update(kw)
    return types.SimpleNamespace(**base)


def _check(plan, dst, shape, axes):
    from pyremap_amd import engine
    return engine.check_field_extents(plan.n_a, plan.n_b, plan.n_b_global,
                                      dst, shape, axes)


#: (shape, remap_axes, dst_grid_dims, the text of the ValueError)
MALFORMED = [
    ((N_A + 1, 12), [0], DST, SRC_TEXT.format(N_A + 1)),
    ((N_A - 1, 12), [0], DST, SRC_TEXT.format(N_A - 1)),
    ((2 * N_A, 12), [0], DST, SRC_TEXT.format(2 * N_A)),
    ((30, 51, 12), [0, 1], DST, SRC_TEXT.format(30 * 51)),
    ((N_A, 12), [0], (19, 60), DST_TEXT.format('19, 60')),
    ((N_A, 12), [0], (38, 61), DST_TEXT.format('38, 61')),
    # the same with the source axes elsewhere
    ((6, N_A + 1, 40), [1], DST, SRC_TEXT.format(N_A + 1)),
    ((6, 40, N_A - 1), [-1], DST, SRC_TEXT.format(N_A - 1)),
    ((6, 30, 4, 51), [1, 3], DST, SRC_TEXT.format(30 * 51)),
    ((6, N_A, 40), [1], (38, 61), DST_TEXT.format('38, 61')),
    # both wrong: the source extent is named first, as remap_tensor did
    ((N_A + 1, 12), [0], (19, 60), SRC_TEXT.format(N_A + 1)),
    # a flat destination that is not n_b
    ((N_A, 12), [0], (N_B + 1,), DST_TEXT.format(N_B + 1)),
    # the wrong axis named
    ((N_A, 12), [1], DST, SRC_TEXT.format(12)),
    ((N_A,), [0], (2, 38, 60), DST_TEXT.format('2, 38, 60')),
]


@pytest.mark.parametrize('shape,axes,dst,text', MALFORMED)
def test_checker_raises_the_two_texts(shape, axes, dst, text):
    with pytest.raises(ValueError, match=text):
        _check(_plan(), dst, shape, axes)


#: (shape, remap_axes, dst_grid_dims, axes returned, dst_shape returned)
WELL_FORMED = [
    ((N_A,), [0], DST, [0], [38, 60]),                     # one source axis
    ((N_A, 12), [0], DST, [0], [38, 60]),                  # leading
    ((6, N_A, 40), [1], DST, [1], [38, 60]),               # middle
    ((6, 40, N_A), [2], DST, [2], [38, 60]),               # trailing
    ((30, 50), [0, 1], DST, [0, 1], [38, 60]),             # two source axes
    ((30, 50, 512), [0, 1], DST, [0, 1], [38, 60]),
    ((6, 30, 50, 4), [1, 2], DST, [1, 2], [38, 60]),
    ((6, 4, 30, 50), [2, 3], DST, [2, 3], [38, 60]),
    ((30, 4, 50), [0, 2], DST, [0, 2], [38, 60]),          # dims between
    ((50, 30), [1, 0], DST, [1, 0], [38, 60]),             # order kept
    ((6, N_A, 40), [-2], DST, [1], [38, 60]),              # negative axes
    ((6, 30, 50), [-2, -1], DST, [1, 2], [38, 60]),
    ((N_A, 12), [0], None, [0], [N_B]),                    # no grid named
    ((N_A, 12), [0], (N_B,), [0], [N_B]),
    ((N_A, 12), [0], (2, 19, 60), [0], [2, 19, 60]),
    ((N_A, 12), [0], [np.int64(38), np.int32(60)], [0], [38, 60]),
]


@pytest.mark.parametrize('shape,axes,dst,want_axes,want_dst', WELL_FORMED)
def test_checker_passes_well_formed_fields(shape, axes, dst, want_axes,
                                           want_dst):
    got_axes, got_dst = _check(_plan(), dst, shape, axes)
    assert got_axes == want_axes
    assert got_dst == want_dst
    assert all(type(d) is int for d in got_dst)


def test_a_row_shard_answers_flat_and_its_grid_is_not_compared():
    """Rows [r0, r1) of the mapping: n_b != n_b_global.  dst_grid_dims names
    the grid of the WHOLE mapping and is not compared, as before; the source
    extent is."""
    shard = _plan(n_b=700, n_b_global=N_B)
    for dst in (DST, (19, 60), None, (700,)):
        assert _check(shard, dst, (6, N_A, 40), [1]) == ([1], [700])
    with pytest.raises(ValueError, match=SRC_TEXT.format(N_A + 1)):
        _check(shard, DST, (6, N_A + 1, 40), [1])


def test_the_two_texts_are_stated_once():
    """Every route raises through the one checker: the words stand in
    engine.py and nowhere else in the package."""
    import glob
    import os
    import pyremap_amd
    root = os.path.dirname(pyremap_amd.__file__)
    for words in ('source cells but', 'do not hold n_b'):
        found = []
        for path in glob.glob(os.path.join(root, '**', '*.py'),
                              recursive=True):
            with open(path, encoding='utf-8') as f:
                found += [path] * f.read().count(words)
        assert [os.path.basename(p) for p in found] == ['engine.py'], words


# -- the routes whose first lines run without a device ------------------------

@pytest.fixture
def doors(monkeypatch):
    """Every door to a raw pointer fails the test when it is reached."""
    from pyremap_amd import engine
    reached = []

    def shut(name):
        def door(*a, **k):
            reached.append(name)
            raise AssertionError(f'{name} reached with a malformed field')
        return door
    for name in ('apply_strided', 'gather_rows', 'scan_nan',
                 'scan_nan_layout', 'load_library'):
        monkeypatch.setattr(engine, name, shut(name))
    return reached


ROUTE_CASES = [(s, a, d, t) for s, a, d, t in MALFORMED[:6]]


@pytest.mark.parametrize('shape,axes,dst,text', ROUTE_CASES)
def test_device_routes_check_before_anything_else(doors, shape, axes, dst,
                                                  text):
    torch = pytest.importorskip('torch')
    from pyremap_amd import engine, parallel
    field = torch.zeros(shape)
    plan = _plan(device=torch.device('cpu'))
    with pytest.raises(ValueError, match=text):
        engine.remap_tensor(plan, dst, field, axes, engine.MODE_FRACB)
    with pytest.raises(ValueError, match=text):
        engine.remap_tensor_auto_mode(plan, dst, field, axes, 0.3)
    # a multi-device plan standing where the plan stands
    multi = object.__new__(parallel.MultiDeviceRemap)
    multi.n_a, multi.n_b, multi.n_b_global = N_A, N_B, N_B
    multi.shards = []
    multi.device = torch.device('meta')      # a move there would not raise
    for call in (
            lambda: multi.remap_tensor(dst, field, axes, engine.MODE_FRACB),
            lambda: multi.remap_tensor_auto_mode(dst, field, axes, 0.3),
            lambda: engine.remap_tensor(multi, dst, field, axes,
                                        engine.MODE_FRACB),
            lambda: engine.remap_tensor_auto_mode(multi, dst, field, axes,
                                                  0.3)):
        with pytest.raises(ValueError, match=text):
            call()
    assert doors == []


def _sharded(torch, parallel):
    sharded = object.__new__(parallel.ShardedRemap)
    sharded._full = _plan()
    sharded.rank, sharded.world_size, sharded.group = 0, 1, None
    sharded.exchange, sharded._logged = 'alltoall', set()
    sharded.ucols = torch.arange(0, N_A, 3, dtype=torch.int32)
    sharded.plan = _plan(device=torch.device('meta'))
    return sharded


@pytest.mark.parametrize('shape,axes,dst,text', ROUTE_CASES)
def test_sharded_routes_check_on_every_rank(doors, shape, axes, dst, text):
    """ShardedRemap.remap_tensor from the tensor and -- a rank that holds no
    data -- from `shape`; distribute and apply_pipelined (row slabs: the
    source extent only)."""
    torch = pytest.importorskip('torch')
    from pyremap_amd import engine, parallel
    sharded = _sharded(torch, parallel)
    field = torch.zeros(shape)
    for mode in ('auto', 'fracb'):
        with pytest.raises(ValueError, match=text):
            sharded.remap_tensor(dst, field, axes, threshold=0.3, mode=mode)
        with pytest.raises(ValueError, match=text):
            sharded.remap_tensor(dst, None, axes, threshold=0.3, mode=mode,
                                 shape=shape, dtype=torch.float64)
    if 'source cells' in text and len(axes) == 1:
        with pytest.raises(ValueError, match=text):
            sharded.distribute(field, axis=axes[0])
        with pytest.raises(ValueError, match=text):
            sharded.distribute(None, axis=axes[0], shape=shape,
                               dtype=torch.float64)
        good = torch.zeros((N_A, 12))
        # a malformed batch anywhere in the list stops the call before the
        # first exchange
        for batches in ([field], [good, field], [good, good, field]):
            with pytest.raises(ValueError, match=text):
                sharded.apply_pipelined(batches, engine.MODE_FRACB)
    assert doors == []


def test_no_runtime_for_2d_copies_is_an_answer_not_an_error(monkeypatch):
    """host_path._hip(): when no HIP runtime loads under any of its names the
    answer is None (the column-panel route declines), asked for once."""
    pytest.importorskip('torch')
    import ctypes
    from pyremap_amd import host_path
    asked = []

    class NoLibrary:
        def __getattr__(self, name):
            return getattr(ctypes, name)

        @staticmethod
        def CDLL(name, *a, **k):
            asked.append(name)
            raise OSError(f'{name}: cannot open shared object file')
    monkeypatch.setattr(host_path, 'ctypes', NoLibrary())
    monkeypatch.setattr(host_path, '_hip_runtime', [None])
    assert host_path._hip() is None
    assert asked[0].endswith('libamdhip64.so') and '/' in asked[0]
    assert 'libamdhip64.so' in asked[1:]          # the bare soname
    assert any(n.startswith('libamdhip64.so.') for n in asked)
    n = len(asked)
    assert host_path._hip() is None and len(asked) == n
