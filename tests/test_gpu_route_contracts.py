"""
Wrong-shaped and wrong-device fields on every route to a launch.

`engine.check_field_extents` states the contract between a field and a
mapping; every route -- the five host routes of `host_path.remap_host_array`
(single upload, column panels, bands, the batch ring, `keep_on_device`),
`remap_host_batch`, the multi-device plan, `ShardedRemap`, `engine.remap_tensor`
and `remap_tensor_auto_mode` -- raises it before its first allocation, thread,
copy or launch.  The table below hands each route each malformation.

The tests are safe on a tree where a check is missing: every door to a raw
pointer (`host_path._copy_2d`, `engine.apply_strided`, `gather_rows`,
`scan_nan`, `scan_nan_layout`) is wrapped; while the guard is armed a wrapper
records the call, raises AssertionError and does NOT execute.  No malformed
call runs without the guard armed.

After every malformed call the same route serves a well-formed field and
equals the oracle (remap_numpy.py:223-297), bit for bit, data and mask: the
route was not left half set up.  No tolerance anywhere.

(The band route needs a source numbering that follows the destination rows --
`_banded_pipeline` declines on the mesh-numbered problem by design -- so its
rows run on the SAME problem numbered `locality='raster'`; every other row on
the mesh-numbered one.)
"""
import ctypes
import gc
import threading

import numpy as np
import pytest

from helpers import assert_bitwise

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

THR = 0.3
SRC_TEXT = 'the remapped axes hold {} source cells but the mapping has ' \
           'n_a = 1500'
DST_TEXT = r'dst_grid_dims \[{}\] do not hold n_b = 2280 cells'


@pytest.fixture(scope='module', autouse=True)
def _settled_collector():
    """The pinned-memory accounting is read after `gc.collect()`, three times
    per cell of the table: collect what earlier modules left behind once,
    then keep the objects alive so far out of the later collections (they
    only walk what the cell itself made)."""
    gc.collect()
    gc.freeze()
    yield
    gc.unfreeze()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'these tests need an MI355X'
    from pyremap_amd import engine
    engine.load_library()
    return torch.device('cuda', 0)


def _problem(dev, locality):
    from oracle import oracle
    from pyremap_amd import engine, synthetic
    m = synthetic.conservative_map(1500, (38, 60), 6, 22, seed=5,
                                   signed=True, locality=locality)
    mm = m.numpy()
    plan = engine.RemapPlan.from_triplets(
        mm['row'], mm['col'], mm['S'], mm['frac_b'], m.n_a, m.n_b,
        index_base=1, device=dev)
    csr = oracle.coo_to_csr(mm['row'] - 1, mm['col'] - 1, mm['S'], m.n_b,
                            m.n_a)
    plan.auto_schedule(m.dst_dims)
    assert (m.n_a, m.n_b, tuple(m.dst_dims)) == (1500, 2280, (38, 60))
    return m, mm, plan, csr


@pytest.fixture(scope='module')
def problem(dev):
    from pyremap_amd import engine
    m, mm, plan, csr = _problem(dev, 'mesh')
    assert engine.cell_mask_form(plan)          # 8-row groups
    return m, mm, plan, csr


@pytest.fixture(scope='module')
def band_problem(dev):
    return _problem(dev, 'raster')


@pytest.fixture(scope='module')
def multi(dev, problem):
    from pyremap_amd.parallel import MultiDeviceRemap
    m, _, plan, _ = problem
    return MultiDeviceRemap(plan, [0, 0], grid_dims=m.dst_dims)


@pytest.fixture(scope='module')
def sharded(problem):
    from pyremap_amd.parallel import ShardedRemap
    m, _, plan, _ = problem
    one = ShardedRemap(plan, grid_dims=m.dst_dims)       # no process group
    assert one.world_size == 1 and one.plan.n_b == plan.n_b
    return one


# -- the guard ---------------------------------------------------------------

class Guard:
    def __init__(self):
        self.armed = False
        self.calls = []          # (door, {n_batch, k_inner} where given)
        self.panel = []          # _panel_pipeline answered? (spy)
        self.banded = []         # _banded_pipeline answered? (spy)

    def reset(self):
        del self.calls[:], self.panel[:], self.banded[:]

    def count(self, name, **kw):
        return sum(1 for n, k in self.calls if n == name and
                   all(k.get(key) == v for key, v in kw.items()))


@pytest.fixture
def guard(monkeypatch):
    from pyremap_amd import engine, host_path
    g = Guard()

    def wrap(mod, name):
        real = getattr(mod, name)

        def door(*a, **k):
            g.calls.append((name, {key: k[key] for key in
                                   ('n_batch', 'k_inner') if key in k}))
            if g.armed:
                raise AssertionError(
                    f'{name} reached while the guard was armed')
            return real(*a, **k)
        monkeypatch.setattr(mod, name, door)

    def spy(name, log):
        real = getattr(host_path, name)

        def route(*a, **k):
            out = real(*a, **k)
            log.append(out is not None)
            return out
        monkeypatch.setattr(host_path, name, route)
    wrap(host_path, '_copy_2d')
    for name in ('apply_strided', 'gather_rows', 'scan_nan',
                 'scan_nan_layout'):
        wrap(engine, name)
    spy('_panel_pipeline', g.panel)
    spy('_banded_pipeline', g.banded)
    yield g
    g.armed = False


# -- the routes --------------------------------------------------------------

def _holed(shape, axis, seed):
    """A field with whole source cells missing (and cell 0 among them)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape)
    gone = rng.random(shape[axis]) < 0.2
    gone[0] = True
    index = [slice(None)] * len(shape)
    index[axis] = gone
    x[tuple(index)] = np.nan
    return x


class Route:
    """One route: how it is forced, called, recognised and what it returns.
    ``call(ctx, field, axes, dims)`` -> (data, mask or None) as numpy, or a
    list of such pairs; ``answered(guard, got)``: did the named route answer
    the well-formed call?"""
    problem = 'problem'
    shape, axis = None, 0
    mode, want_mask = 'masked', True
    slabs = False                 # returns row slabs: no dst_grid_dims rows
    CHUNK_BYTES = None

    def __init__(self, name, **kw):
        self.name = name
        for k, v in kw.items():
            setattr(self, k, v)

    def __repr__(self):
        return self.name

    def force(self, monkeypatch, m):
        from pyremap_amd import host_path
        if self.CHUNK_BYTES is not None:
            monkeypatch.setattr(host_path, 'CHUNK_BYTES',
                                self.CHUNK_BYTES(m)
                                if callable(self.CHUNK_BYTES)
                                else self.CHUNK_BYTES)

    def field(self, shape):
        """Data for a field of ``shape`` (well-formed or not)."""
        x = _holed(shape, self.axis, 11)
        if self.mode == 'fracb':
            x = np.nan_to_num(x, nan=0.5)
        return x

    def masked(self, field):
        return self.mode == 'masked' or (
            self.mode == 'auto' and bool(np.isnan(field).any()))


def _host(ctx, route, field, axes, dims, plan=None, **kw):
    from pyremap_amd import host_path
    pending = host_path.remap_host_array(
        plan if plan is not None else ctx['plan'], dims, field, axes,
        mode=route.mode, threshold=None if route.mode == 'fracb' else THR,
        want_mask=route.want_mask, **kw)
    ctx['pending'] = type(pending).__name__
    got = pending.result()
    return (got[0], got[1]) if route.want_mask else (got, None)


def _numpy(res, want_mask):
    if want_mask:
        return res[0].cpu().numpy(), res[1].cpu().numpy().astype(bool)
    return res.cpu().numpy(), None


class Single(Route):
    shape = (1500, 12)

    def call(self, ctx, field, axes, dims):
        return _host(ctx, self, field, axes, dims)

    def answered(self, g, ctx):
        return g.panel == [] and g.banded == [] and \
            g.count('_copy_2d') == 0 and \
            g.count('apply_strided', n_batch=1, k_inner=12) >= 1


class Panels(Route):
    shape = (1500, 512)
    CHUNK_BYTES = 1 << 16

    def call(self, ctx, field, axes, dims):
        return _host(ctx, self, field, axes, dims)

    def answered(self, g, ctx):
        # four panels: one 2-D copy up and one (two with a mask) down each
        return g.panel == [True] and g.banded == [] and \
            g.count('_copy_2d') == 4 * (3 if self.want_mask else 2) and \
            g.count('apply_strided', n_batch=1, k_inner=128) >= 4


class Banded(Route):
    problem = 'band_problem'
    shape = (1500, 70)
    CHUNK_BYTES = 96 * 1024

    def call(self, ctx, field, axes, dims):
        return _host(ctx, self, field, axes, dims)

    def answered(self, g, ctx):
        # too few panels: the panel route declines first
        return g.panel == [False] and g.banded == [True] and \
            g.count('apply_strided', n_batch=1, k_inner=70) >= 2


class Ring(Route):
    shape, axis = (6, 1500, 40), 1

    @staticmethod
    def CHUNK_BYTES(m):
        return 2 * max(m.n_a, m.n_b) * 40 * 8          # two batches wide

    def call(self, ctx, field, axes, dims):
        return _host(ctx, self, field, axes, dims)

    def answered(self, g, ctx):
        return g.panel == [] and g.banded == [] and \
            g.count('apply_strided', n_batch=2, k_inner=40) >= 3 and \
            g.count('apply_strided', n_batch=6) == 0


class Keep(Route):
    shape = (1500, 12)
    mode, want_mask = 'auto', False

    def call(self, ctx, field, axes, dims):
        return _host(ctx, self, field, axes, dims, keep_on_device=True)

    def answered(self, g, ctx):
        return ctx['pending'] == 'OnDevice' and g.panel == [] and \
            g.count('apply_strided') >= 1


class Batch(Route):
    """remap_host_batch: three (1, n_a) arrays, one of them with NaNs."""
    shape, axis = (1, 1500), 1
    mode, want_mask = 'auto', False

    def arrays(self, field):
        second = np.nan_to_num(field, nan=-2.0) * 3.0
        return [field, second, second[:, ::-1].copy()]

    def call(self, ctx, field, axes, dims):
        from pyremap_amd import host_path
        pending = host_path.remap_host_batch(
            ctx['plan'], dims, self.arrays(field), axes, mode='auto',
            threshold=THR)
        ctx['pending'] = type(pending).__name__
        return [(a, None) for a in pending.result()]

    def answered(self, g, ctx):
        return ctx['pending'] == 'PendingBatch' and \
            g.count('apply_strided') >= 2 and g.panel == []


class MultiTensor(Route):
    shape, axis = (3, 1500, 24), 1

    def call(self, ctx, field, axes, dims):
        from pyremap_amd import engine
        fd = torch.from_numpy(field).to(ctx['dev'])
        return _numpy(engine.remap_tensor(
            ctx['multi'], dims, fd, axes, engine.MODE_MASKED, threshold=THR,
            want_mask=True), True)

    def answered(self, g, ctx):
        return g.count('gather_rows') == 2 and g.count('scan_nan_layout') == 0


class MultiAuto(Route):
    shape, axis = (3, 1500, 24), 1
    mode, want_mask = 'auto', False

    def call(self, ctx, field, axes, dims):
        from pyremap_amd import engine
        fd = torch.from_numpy(field).to(ctx['dev'])
        return _numpy(engine.remap_tensor_auto_mode(
            ctx['multi'], dims, fd, axes, THR), False)

    def answered(self, g, ctx):
        return g.count('gather_rows') == 2 and g.count('scan_nan_layout') == 1


class MultiHost(Route):
    shape = (1500, 12)

    def call(self, ctx, field, axes, dims):
        return _host(ctx, self, field, axes, dims, plan=ctx['multi'])

    def answered(self, g, ctx):
        return g.count('gather_rows') == 2 and g.panel == []


class ShardedTensor(Route):
    shape, axis = (3, 1500, 24), 1
    mode = 'auto'

    def call(self, ctx, field, axes, dims):
        fd = torch.from_numpy(field).to(ctx['dev'])
        return _numpy(ctx['sharded'].remap_tensor(
            dims, fd, axes, threshold=THR, mode='auto', want_mask=True), True)

    def answered(self, g, ctx):
        return g.count('gather_rows') == 1 and g.count('scan_nan_layout') == 1


class ShardedDistribute(Route):
    shape = (1500, 24)
    slabs = True

    def call(self, ctx, field, axes, dims):
        from pyremap_amd import engine
        assert len(axes) == 1
        sharded = ctx['sharded']
        fd = torch.from_numpy(field).to(ctx['dev'])
        packed = sharded.distribute(fd, axis=axes[0])
        return _numpy(sharded.apply(packed, axes, engine.MODE_MASKED,
                                    threshold=THR, want_mask=True), True)

    def answered(self, g, ctx):
        return g.count('gather_rows') == 1


class ShardedPipelined(Route):
    shape = (1500, 24)
    mode, want_mask = 'fracb', False
    slabs = True

    def call(self, ctx, field, axes, dims):
        from pyremap_amd import engine
        assert list(axes) == [0]
        fd = torch.from_numpy(field).to(ctx['dev'])
        # the malformed batch comes LAST: nothing of the good one may run
        good = torch.zeros((1500, 24), dtype=torch.float64,
                           device=ctx['dev'])
        batches = [fd, fd] if tuple(fd.shape) == self.shape else [good, fd]
        outs = ctx['sharded'].apply_pipelined(batches, engine.MODE_FRACB)
        return [_numpy(y, False) for y in outs]

    def answered(self, g, ctx):
        return g.count('gather_rows') == 2


class Tensor(Route):
    shape, axis = (3, 1500, 24), 1

    def call(self, ctx, field, axes, dims):
        from pyremap_amd import engine
        fd = torch.from_numpy(field).to(ctx['dev'])
        return _numpy(engine.remap_tensor(
            ctx['plan'], dims, fd, axes, engine.MODE_MASKED, threshold=THR,
            want_mask=True), True)

    def answered(self, g, ctx):
        return g.count('apply_strided') >= 1 and g.count('gather_rows') == 0


class TensorAuto(Route):
    shape, axis = (3, 1500, 24), 1
    mode, want_mask = 'auto', False

    def call(self, ctx, field, axes, dims):
        from pyremap_amd import engine
        fd = torch.from_numpy(field).to(ctx['dev'])
        return _numpy(engine.remap_tensor_auto_mode(
            ctx['plan'], dims, fd, axes, THR), False)

    def answered(self, g, ctx):
        # (8-row groups: the layout-aware scan, then the gated launches)
        return g.count('scan_nan_layout') + g.count('scan_nan') == 1 and \
            g.count('apply_strided') >= 2


ROUTES = [
    Single('single upload'),
    Panels('panels fracb', mode='fracb'),
    Panels('panels masked', mode='masked'),
    Panels('panels auto', mode='auto', want_mask=False),
    Banded('banded fracb', mode='fracb'),
    Banded('banded masked', mode='masked'),
    Ring('ring'),
    Keep('keep_on_device'),
    Batch('remap_host_batch'),
    MultiTensor('multi-device remap_tensor'),
    MultiAuto('multi-device remap_tensor_auto_mode'),
    MultiHost('multi-device remap_host_array'),
    ShardedTensor('sharded remap_tensor'),
    ShardedDistribute('sharded distribute'),
    ShardedPipelined('sharded apply_pipelined'),
    Tensor('engine.remap_tensor'),
    TensorAuto('engine.remap_tensor_auto_mode'),
]

MALFORMATIONS = ['n_a + 1', 'n_a - 1', '2 n_a', '(30, 51)', 'dst (19, 60)',
                 'dst (38, 61)']

TABLE = [pytest.param(r, bad, id=f'{r.name}-{bad}')
         for r in ROUTES for bad in MALFORMATIONS
         if not (r.slabs and bad.startswith('dst'))]


def _malformed(route, bad, dims):
    """(shape, axes, dst_grid_dims, text) of one cell of the table."""
    shape, ax = list(route.shape), route.axis
    if bad.startswith('dst'):
        wrong = (19, 60) if bad == 'dst (19, 60)' else (38, 61)
        return tuple(shape), [ax], wrong, \
            DST_TEXT.format(f'{wrong[0]}, {wrong[1]}')
    if bad == '(30, 51)':
        shape[ax:ax + 1] = [30, 51]
        if route.slabs:
            # one axis is all these routes take: the first of the two
            return tuple(shape), [ax], dims, SRC_TEXT.format(30)
        return tuple(shape), [ax, ax + 1], dims, SRC_TEXT.format(30 * 51)
    n = {'n_a + 1': 1501, 'n_a - 1': 1499, '2 n_a': 3000}[bad]
    shape[ax] = n
    return tuple(shape), [ax], dims, SRC_TEXT.format(n)


_REFERENCES = {}


def _reference(route, probs):
    """The oracle's answer to the route's well-formed field, computed once
    and left unchanged: (field, [(data, mask), ...])."""
    if route.name not in _REFERENCES:
        from oracle import oracle
        m, mm, _, csr = probs[route.problem]
        field = route.field(route.shape)
        fields = route.arrays(field) if isinstance(route, Batch) else [field]
        refs = []
        for f in fields:
            masked = route.masked(f)
            arg = np.ma.masked_array(f, np.isnan(f)) if masked else f
            ref = oracle.remap_numpy_array(
                csr, mm['frac_b'], m.dst_dims, arg, [route.axis],
                THR if masked else None)
            data, mask = np.ma.filled(ref, np.nan), np.ma.getmaskarray(ref)
            if route.slabs:
                data = data.reshape(m.n_b, -1)
                mask = mask.reshape(m.n_b, -1)
            data.setflags(write=False)
            mask.setflags(write=False)
            refs.append((data, mask))
        if isinstance(route, ShardedPipelined):
            refs = refs * 2
        field.setflags(write=False)
        _REFERENCES[route.name] = field, refs
    return _REFERENCES[route.name]


def _well_formed(route, ctx, guard, probs, what):
    """The route serves a well-formed field: the named route answers and the
    result is the oracle's, data and mask."""
    m = probs[route.problem][0]
    field, refs = _reference(route, probs)
    guard.armed = False
    guard.reset()
    got = route.call(ctx, field.copy(), [route.axis], m.dst_dims)
    assert route.answered(guard, ctx), \
        (what, guard.calls, guard.panel, guard.banded)
    got = got if isinstance(got, list) else [got]
    assert len(got) == len(refs)
    for i, ((data, mask), (ref, ref_mask)) in enumerate(zip(got, refs)):
        assert_bitwise(data, ref, f'{what} [{i}]')
        if mask is not None:
            assert np.array_equal(np.asarray(mask, dtype=bool), ref_mask), \
                f'{what} [{i}] mask'


def _route_threads():
    return [t.name for t in threading.enumerate()
            if t.name.startswith('pyremap_amd.')]


@pytest.fixture
def ctx(dev, problem, band_problem, multi, sharded):
    return {'dev': dev, 'multi': multi, 'sharded': sharded,
            'probs': {'problem': problem, 'band_problem': band_problem}}


@pytest.mark.parametrize('route,bad', TABLE)
def test_route_rejects_malformed_field(ctx, guard, monkeypatch, route, bad):
    from pyremap_amd import host_path
    probs = ctx['probs']
    m, _, plan, _ = probs[route.problem]
    ctx['plan'] = plan
    route.force(monkeypatch, m)
    shape, axes, dims, text = _malformed(route, bad, m.dst_dims)
    field = route.field(shape)
    base = host_path.pinned_bytes_alive()
    n_threads = threading.active_count()
    guard.reset()
    guard.armed = True                  # from here to the end of the call
    try:
        with pytest.raises(ValueError, match=text):
            route.call(ctx, field, axes, dims)
    finally:
        guard.armed = False
    assert guard.calls == [], 'a door to a raw pointer was reached'
    assert guard.panel == [] and guard.banded == []
    assert _route_threads() == []
    assert threading.active_count() == n_threads
    gc.collect()
    assert host_path.pinned_bytes_alive() == base
    # not left half set up: the same route, a well-formed field, the oracle
    _well_formed(route, ctx, guard, probs, f'{route.name} after {bad}')
    assert _route_threads() == []
    gc.collect()
    assert host_path.pinned_bytes_alive() == base


# -- well-formed neighbours of the new derivation of K ----------------------

def _host_case(plan, csr, mm, dims, field, axes, mode, want_mask, what):
    from oracle import oracle
    from pyremap_amd import host_path
    masked = mode == 'masked' or (mode == 'auto' and
                                  bool(np.isnan(field).any()))
    arg = np.ma.masked_array(field, np.isnan(field)) if masked else field
    ref = oracle.remap_numpy_array(csr, mm['frac_b'], dims, arg, axes,
                                   THR if masked else None)
    got = host_path.remap_host_array(
        plan, dims, field, axes, mode=mode,
        threshold=None if mode == 'fracb' else THR,
        want_mask=want_mask).result()
    data = got[0] if want_mask else got
    assert_bitwise(data, np.ma.filled(ref, np.nan), what)
    if want_mask:
        assert np.array_equal(got[1], np.ma.getmaskarray(ref)), what


def test_panels_take_k_from_the_trailing_dims(guard, monkeypatch, problem):
    """Column panels on fields whose K is a product of several trailing dims
    or follows two source axes; a last panel of ONE column; exactly PANEL_MIN
    panels, and one fewer (declined); float32 in the masked mode with its
    mask, and in mode 'auto' with one NaN off the strided sample (the device
    scans meet it: the masked mode over again, `recheck`)."""
    from pyremap_amd import host_path
    m, mm, plan, csr = problem
    monkeypatch.setattr(host_path, 'CHUNK_BYTES', 1 << 16)
    kp, least = host_path.PANEL_COLUMNS, host_path.PANEL_MIN
    assert (kp, least) == (128, 3)
    cases = [
        ('3-D (n_a, 16, 32)', (m.n_a, 16, 32), [0], np.float64, True),
        ('(30, 50, 512), two source axes', (30, 50, 512), [0, 1], np.float64,
         True),
        ('last panel of one column', (m.n_a, 2 * kp + 1), [0], np.float64,
         True),
        ('exactly PANEL_MIN panels', (m.n_a, least * kp), [0], np.float64,
         True),
        ('one panel fewer than PANEL_MIN', (m.n_a, (least - 1) * kp), [0],
         np.float64, False),
    ]
    for tag, shape, axes, dtype, takes in cases:
        holed = _holed(shape, 0, 23).astype(dtype)
        plain = np.nan_to_num(holed, nan=1.5)
        for field, mode, want_mask in ((plain, 'fracb', True),
                                       (holed, 'masked', True),
                                       (holed, 'auto', False)):
            guard.reset()
            _host_case(plan, csr, mm, m.dst_dims, field, axes, mode,
                       want_mask, f'{tag} {mode}')
            assert guard.panel == [takes], (tag, mode, guard.panel)
            K = int(np.prod(shape[len(axes):]))
            n_p = -(-K // kp)
            if takes:
                assert guard.count('_copy_2d') == \
                    n_p * (3 if want_mask else 2), (tag, mode)
                assert guard.count('apply_strided', k_inner=K - (n_p - 1) *
                                   kp) >= 1, (tag, mode)
            else:
                assert guard.count('_copy_2d') == 0
    # float32 meets the panels in the masked and the auto mode too
    x32 = _holed((m.n_a, 512), 0, 29).astype(np.float32)
    guard.reset()
    _host_case(plan, csr, mm, m.dst_dims, x32, [0], 'masked', True,
               'float32 masked')
    assert guard.panel == [True]
    rare = np.nan_to_num(x32, nan=0.25)
    rare[m.n_a // 2 + 1, 512 - 3] = np.nan             # off the sample
    assert not host_path._sampled_nan(rare)
    guard.reset()
    _host_case(plan, csr, mm, m.dst_dims, rare, [0], 'auto', False,
               'float32 auto, one NaN off the sample')
    assert guard.panel == [True]
    # four panels scanned, launched in the frac_b mode, then again masked
    assert guard.count('scan_nan') == 4
    assert guard.count('apply_strided', k_inner=128) >= 8
    assert guard.count('_copy_2d') == 4 * 3


def test_bands_take_k_from_the_trailing_dims(guard, monkeypatch,
                                             band_problem):
    from pyremap_amd import host_path
    m, mm, plan, csr = band_problem
    monkeypatch.setattr(host_path, 'CHUNK_BYTES', 96 * 1024)
    holed = _holed((m.n_a, 7, 10), 0, 31)
    for field, mode in ((np.nan_to_num(holed, nan=1.5), 'fracb'),
                        (holed, 'masked')):
        guard.reset()
        _host_case(plan, csr, mm, m.dst_dims, field, [0], mode, True,
                   f'banded (n_a, 7, 10) {mode}')
        assert guard.panel == [False] and guard.banded == [True]
        assert guard.count('apply_strided', k_inner=70) >= 2


# -- ShardedRemap, any device the field lives on ------------------------------

def _sharded_auto(problem, sharded, tensor, field64, what):
    from oracle import oracle
    m, mm, _, csr = problem
    masked = bool(np.isnan(field64).any())
    arg = np.ma.masked_array(field64, np.isnan(field64)) if masked \
        else field64
    ref = oracle.remap_numpy_array(csr, mm['frac_b'], m.dst_dims, arg, [1],
                                   THR if masked else None)
    y, mask = sharded.remap_tensor(m.dst_dims, tensor, [1], threshold=THR,
                                   mode='auto', want_mask=True)
    assert y.device == sharded.plan.device and y.dtype == torch.float64
    assert_bitwise(y.cpu().numpy(), np.ma.filled(ref, np.nan), what)
    assert np.array_equal(mask.cpu().numpy().astype(bool),
                          np.ma.getmaskarray(ref)), what


def test_sharded_auto_takes_a_field_from_anywhere(dev, problem, sharded):
    """World size 1, mode 'auto', NaNs in whole cells: a CPU tensor, a
    float32 device tensor, an int32 device tensor (no NaN can live in it: the
    frac_b branch, scipy's upcast to float64)."""
    m = problem[0]
    x = _holed((3, m.n_a, 24), 1, 37)
    _sharded_auto(problem, sharded, torch.from_numpy(x), x, 'CPU tensor')
    x32 = x.astype(np.float32)
    _sharded_auto(problem, sharded, torch.from_numpy(x32).to(dev),
                  x32.astype(np.float64), 'float32 device tensor')
    xi = np.rint(np.nan_to_num(x, nan=7.0) * 100.0).astype(np.int32)
    _sharded_auto(problem, sharded, torch.from_numpy(xi).to(dev),
                  xi.astype(np.float64), 'int32 device tensor')


@pytest.mark.skipif(torch.cuda.device_count() < 2,
                    reason='needs two physical GPUs')
def test_sharded_auto_takes_a_field_from_another_gpu(problem, sharded):
    m = problem[0]
    x = _holed((3, m.n_a, 24), 1, 41)
    _sharded_auto(problem, sharded,
                  torch.from_numpy(x).to(torch.device('cuda', 1)), x,
                  'tensor on cuda:1')


# -- ADVICE items 2 and 3 ------------------------------------------------------

def test_panels_without_torchs_own_hip_runtime(guard, monkeypatch, problem):
    """host_path._hip(): torch's lib directory holds no loadable runtime (a
    torch built against a system ROCm).  The runtime is found under its
    soname, or the panel route declines -- never an OSError out of the
    uploader thread -- and the result is the oracle's either way."""
    from pyremap_amd import host_path
    m, mm, plan, csr = problem
    asked = []

    class NotInTorch:
        def __getattr__(self, name):
            return getattr(ctypes, name)

        @staticmethod
        def CDLL(name, *a, **k):
            asked.append(name)
            if '/' in str(name):
                raise OSError(f'{name}: cannot open shared object file')
            return ctypes.CDLL(name, *a, **k)
    monkeypatch.setattr(host_path, 'ctypes', NotInTorch())
    monkeypatch.setattr(host_path, 'CHUNK_BYTES', 1 << 16)
    monkeypatch.setattr(host_path, '_hip_runtime', [None])   # and back after
    holed = _holed((m.n_a, 512), 0, 43)
    for field, mode, want_mask in ((np.nan_to_num(holed, nan=1.5), 'fracb',
                                    True), (holed, 'masked', True)):
        guard.reset()
        _host_case(plan, csr, mm, m.dst_dims, field, [0], mode, want_mask,
                   f'no runtime in torch/lib, {mode}')
        assert guard.panel in ([True], [False])
        found = host_path._hip() is not None
        assert guard.panel == [found]
        assert (guard.count('_copy_2d') > 0) == found
    # looked for once, torch's own path first
    assert asked and '/' in asked[0] and asked[0].endswith('libamdhip64.so')
    assert 'libamdhip64.so' in asked[1:]
    assert _route_threads() == []


def test_panels_decline_beyond_the_device_fraction(guard, monkeypatch,
                                                   problem):
    """Source, result and mask panels stay resident until the result is
    asked for: beyond DEVICE_FRACTION of the free memory the route declines
    and the plain form answers."""
    from pyremap_amd import host_path
    m, mm, plan, csr = problem
    monkeypatch.setattr(host_path, 'CHUNK_BYTES', 1 << 16)
    holed = _holed((m.n_a, 512), 0, 47)
    plain = np.nan_to_num(holed, nan=1.5)
    for fraction, takes in ((0.0, False), (0.5, True)):
        monkeypatch.setattr(host_path, 'DEVICE_FRACTION', fraction)
        for field, mode, want_mask in ((plain, 'fracb', True),
                                       (plain, 'auto', False),
                                       (holed, 'auto', False)):
            guard.reset()
            _host_case(plan, csr, mm, m.dst_dims, field, [0], mode,
                       want_mask, f'DEVICE_FRACTION {fraction} {mode}')
            assert guard.panel == [takes], (fraction, mode, guard.panel)
            assert (guard.count('_copy_2d') > 0) == takes
