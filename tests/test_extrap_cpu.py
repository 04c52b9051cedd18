"""
Nearest-point extrapolation of bilinear and patch maps (ESMF's
--extrap_method neareststod | nearestidavg) without a GPU:
pyremap_amd.weights.nearest_k (the numpy statement of remap_nearest_k),
extrap_rows, extrapolate, and the way make_weights / write_weights / Remapper
hand the three options on.

Bounds.  nearest_k against a plain double loop over Python floats (IEEE
doubles, the same operations in the same order): equality.  extrap_rows:
equality where the issue's definition is an expression (p = 2, p = 0, a
coincident source); a row's weights sum to 1 within 3 * k * 2**-53 -- k
divisions and k - 1 additions, each rounded once (the sum W of the k weights
carries at most (k - 1) u, every quotient w / W one more u, u = 2**-53, so
the exact sum of the quotients is within k u of 1 to first order); the test
adds the weights up with math.fsum, which adds no rounding of its own.
"""
import fnmatch
import math
import os
import re

import numpy as np
import pytest

from helpers import REPO
from test_nearest_cpu import brute, mesh_points, qu240, unit

U = 2.0 ** -53


def loop_nearest_k(S, P, k):
    """The definition, one pair at a time."""
    idx = np.full((len(P), k), -1, dtype=np.int32)
    d2 = np.full((len(P), k), np.inf)
    for i, p in enumerate(P.tolist()):
        pairs = []
        for j, s in enumerate(S.tolist()):
            dx, dy, dz = s[0] - p[0], s[1] - p[1], s[2] - p[2]
            pairs.append(((dx * dx + dy * dy) + dz * dz, j))
        pairs.sort()
        for slot, (d, j) in enumerate(pairs[:k]):
            idx[i, slot], d2[i, slot] = j, d
    return idx, d2


# ---------------------------------------------------------------------------
# 1. nearest_k
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('n_src, k', [(40, 1), (40, 3), (40, 16), (5, 8),
                                      (5, 5), (1, 4)])
def test_nearest_k_is_the_double_loop(n_src, k):
    from pyremap_amd import weights
    rng = np.random.default_rng(n_src + k)
    S = rng.standard_normal((n_src, 3))
    S[n_src // 2:] = S[:n_src - n_src // 2]      # duplicate sources
    P = rng.standard_normal((30, 3))
    P[0] = S[0]                                  # d2 == 0, and a tie
    P[1] = 0.5 * (S[0] + S[-1])
    want_i, want_d = loop_nearest_k(S, P, k)
    for chunk in (7, 512):
        idx, d2 = weights.nearest_k(S, P, k, chunk=chunk)
        assert idx.dtype == np.int32 and d2.dtype == np.float64
        assert idx.shape == d2.shape == (30, k)
        assert np.array_equal(idx, want_i)
        assert d2.tobytes() == want_d.tobytes()
    if k > n_src:
        assert np.all(idx[:, n_src:] == -1) and np.all(d2[:, n_src:] == np.inf)
        assert np.all(idx[:, :n_src] >= 0)
    if n_src > 1:
        assert d2[0, 0] == 0.0 and idx[0, 0] == 0


def test_nearest_k_first_column_is_the_nearest_and_empty_is_served():
    from pyremap_amd import weights
    rng = np.random.default_rng(5)
    S, P = rng.standard_normal((40, 3)), rng.standard_normal((30, 3))
    idx, _ = weights.nearest_k(S, P, 4)
    assert np.array_equal(idx[:, 0], brute(S, P))
    idx, d2 = weights.nearest_k(S, P[:0], 4)
    assert idx.shape == d2.shape == (0, 4)
    for k in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match='from 1 to 16'):
            weights.nearest_k(S, P, k)
    with pytest.raises(ValueError, match='at least one source'):
        weights.nearest_k(S[:0], P, 2)
    with pytest.raises(ValueError, match=r'\(n, 3\)'):
        weights.nearest_k(S[:, :2], P, 2)


# ---------------------------------------------------------------------------
# 2. extrap_rows
# ---------------------------------------------------------------------------

def _lists(rng, n, k, n_src=50):
    from pyremap_amd import weights
    return weights.nearest_k(rng.standard_normal((n_src, 3)),
                             rng.standard_normal((n, 3)), k)


def test_neareststod_rows():
    from pyremap_amd import weights
    idx, d2 = _lists(np.random.default_rng(1), 20, 5)
    row, col, S = weights.extrap_rows(idx, d2, 'neareststod', 2.0)
    assert np.array_equal(row, np.arange(20))
    assert np.array_equal(col, idx[:, 0])
    assert np.all(S == 1.0) and len(S) == 20


def test_a_coincident_source_takes_everything():
    from pyremap_amd import weights
    idx = np.array([[4, 2, 7], [1, 5, 9], [3, -1, -1]], dtype=np.int32)
    d2 = np.array([[0.0, 0.0, 0.5], [0.25, 1.0, 4.0], [0.0, np.inf, np.inf]])
    for p in (0.0, 1.0, 2.0):
        row, col, S = weights.extrap_rows(idx, d2, 'nearestidavg', p)
        assert list(row) == [0, 1, 1, 1, 2]
        assert list(col) == [4, 1, 5, 9, 3]
        assert S[0] == 1.0 and S[4] == 1.0
    row, col, S = weights.extrap_rows(idx, d2, 'nearestidavg', 2.0)
    w = np.array([4.0, 1.0, 0.25])
    assert np.array_equal(S[1:4], w / w.sum())


def test_exponent_two_is_inverse_d2_and_zero_is_the_mean():
    from pyremap_amd import weights
    idx, d2 = _lists(np.random.default_rng(2), 40, 8)
    row, col, S = weights.extrap_rows(idx, d2, 'nearestidavg', 2.0)
    w = 1.0 / d2
    assert np.array_equal(S.reshape(40, 8), w / w.sum(axis=1, keepdims=True))
    assert np.array_equal(row, np.repeat(np.arange(40), 8))
    assert np.array_equal(col.reshape(40, 8), idx)
    # p = 0: the plain mean, over the valid slots where k > n_src
    idx, d2 = _lists(np.random.default_rng(3), 10, 8, n_src=5)
    row, col, S = weights.extrap_rows(idx, d2, 'nearestidavg', 0.0)
    assert len(S) == 50 and np.all(S == 1.0 / 5.0)
    assert np.array_equal(col.reshape(10, 5), idx[:, :5])
    idx, d2 = _lists(np.random.default_rng(4), 10, 7)
    assert np.all(weights.extrap_rows(idx, d2, 'nearestidavg', 0.0)[2] ==
                  1.0 / 7.0)


@pytest.mark.parametrize('p', [0.0, 1.0, 2.0, 3.5])
def test_row_sums(p):
    from pyremap_amd import weights
    worst = 0.0
    for k in range(1, 17):
        idx, d2 = _lists(np.random.default_rng(10 + k), 64, k, n_src=12)
        row, col, S = weights.extrap_rows(idx, d2, 'nearestidavg', p)
        assert np.all(S > 0.0)
        for r in range(64):
            err = abs(math.fsum(S[row == r]) - 1.0)
            worst = max(worst, err / (3 * k * U))
            assert err <= 3 * k * U
    print('p', p, 'worst row-sum error / bound', worst)


def test_extrap_rows_arguments():
    from pyremap_amd import weights
    idx, d2 = _lists(np.random.default_rng(1), 4, 3)
    with pytest.raises(ValueError, match='neareststod.*nearestidavg'):
        weights.extrap_rows(idx, d2, 'creep', 2.0)
    for p in (-1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match='dist_exponent'):
            weights.extrap_rows(idx, d2, 'nearestidavg', p)
    with pytest.raises(ValueError, match=r'\(n, k\)'):
        weights.extrap_rows(idx, d2[:, :2], 'neareststod', 2.0)


# ---------------------------------------------------------------------------
# 3. end to end through the numpy paths
# ---------------------------------------------------------------------------

def _stereo():
    from pyremap_amd.polar import get_polar_descriptor
    return get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0,
                                projection='antarctic')


def _pairs():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return {'qu240': (qu240(), get_lat_lon_descriptor(10.0, 10.0), 251),
            'stereo': (_stereo(), get_lat_lon_descriptor(10.0, 10.0), 548)}


@pytest.fixture(scope='module')
def maps():
    """Per pair: the descriptors, the plain bilinear map and the two
    extrapolated ones, all made once, without the GPU."""
    from pyremap_amd import weights
    patch = pytest.MonkeyPatch()
    patch.setattr(weights, '_gpu_present', lambda: False)
    out = {}
    try:
        for name, (src, dst, n_empty) in _pairs().items():
            made = {None: weights.make_weights(src, dst, 'bilinear')}
            for method in weights.EXTRAP_METHODS:
                made[method] = weights.make_weights(
                    src, dst, 'bilinear', extrap_method=method)
            out[name] = (src, dst, n_empty, made)
    finally:
        patch.undo()
    return out


def _source_points(name, src):
    """Unit vectors of the source's points in the numbering of col, made
    without weights._cell_centres for the grid."""
    if name == 'qu240':
        return unit(*mesh_points(src))
    x, y = np.asarray(src.x), np.asarray(src.y)
    iy, ix = np.divmod(np.arange(len(x) * len(y)), len(x))
    lat, lon = src.project_to_lat_lon(x[ix], y[iy])
    return unit(np.radians(lat), np.radians(lon))


@pytest.mark.parametrize('method', ['neareststod', 'nearestidavg'])
@pytest.mark.parametrize('name', ['qu240', 'stereo'])
def test_every_point_is_mapped_and_the_rest_is_untouched(maps, name, method):
    from pyremap_amd import weights
    from test_nearest_cpu import latlon_centres
    src, dst, n_empty, made = maps[name]
    plain, full = made[None], made[method]
    n_b = 648
    had = np.bincount(plain.row - 1, minlength=n_b) > 0
    assert plain.n_b == n_b and (~had).sum() == n_empty
    assert np.array_equal(plain.frac_b, had.astype(np.float64))
    # every row has an entry now, frac_b is 1
    assert np.all(np.bincount(full.row - 1, minlength=n_b) > 0)
    assert np.all(full.frac_b == 1.0) and len(full.frac_b) == n_b
    assert full.n_a == plain.n_a and full.n_b == n_b
    assert np.array_equal(full.src_grid_dims, plain.src_grid_dims)
    assert np.array_equal(full.dst_grid_dims, plain.dst_grid_dims)
    assert full.row.dtype == np.int32 and full.col.dtype == np.int32
    # rows that were mapped: bit for bit
    old = had[full.row - 1]
    assert np.array_equal(full.row[old], plain.row)
    assert np.array_equal(full.col[old], plain.col)
    assert full.S[old].tobytes() == plain.S.tobytes()
    # sorted by (row, col)
    r, c = full.row.astype(np.int64), full.col.astype(np.int64)
    assert np.all((r[1:] > r[:-1]) | ((r[1:] == r[:-1]) & (c[1:] >= c[:-1])))
    # the new rows
    S = _source_points(name, src)
    assert len(S) == full.n_a
    P = unit(*latlon_centres(10.0))
    empty = np.nonzero(~had)[0]
    new_row, new_col, new_S = full.row[~old], full.col[~old], full.S[~old]
    nearest = brute(S, P[empty])
    if method == 'neareststod':
        assert np.array_equal(new_row - 1, empty)
        assert np.array_equal(new_col - 1, nearest)
        assert np.all(new_S == 1.0)
    else:
        idx, d2 = weights.nearest_k(S, P[empty], 8)
        assert np.array_equal(idx[:, 0], nearest)
        assert np.array_equal(new_row - 1, np.repeat(empty, 8))
        assert np.array_equal(new_col.reshape(-1, 8) - 1, np.sort(idx, axis=1))
        for row in new_S.reshape(-1, 8):
            assert abs(math.fsum(row) - 1.0) <= 3 * 8 * U
        # the nearest of the eight weighs most
        where = np.argmax(new_S.reshape(-1, 8), axis=1)
        assert np.array_equal(
            np.take_along_axis(new_col.reshape(-1, 8), where[:, None], 1)[:, 0]
            - 1, nearest)
    # geometry as for the plain map
    assert full.frac_a is not None and np.all(full.frac_a == 0.0)
    assert np.array_equal(full.area_b, plain.area_b)


@pytest.mark.parametrize('name', ['qu240', 'stereo'])
def test_idempotent_on_a_complete_map(maps, name, monkeypatch):
    from pyremap_amd import weights
    monkeypatch.setattr(weights, '_gpu_present', lambda: False)
    src, dst, _, made = maps[name]
    src_ll = weights._centres_of(src, 'source')
    dst_ll = weights._centres_of(dst, 'destination')
    for method in weights.EXTRAP_METHODS:
        full = made[method]
        again = weights.extrapolate(full, *src_ll, *dst_ll, method)
        for key in ('row', 'col', 'S', 'frac_b'):
            assert np.array_equal(getattr(again, key), getattr(full, key))
    # and by hand from the plain map: the statement of extrapolate
    plain = made[None]
    by_hand = weights.extrapolate(plain, *src_ll, *dst_ll, 'nearestidavg',
                                  num_src_pnts=8, dist_exponent=2.0)
    for key in ('row', 'col', 'S', 'frac_b'):
        assert np.array_equal(getattr(by_hand, key),
                              getattr(made['nearestidavg'], key))
    three = weights.extrapolate(plain, *src_ll, *dst_ll, 'nearestidavg',
                                num_src_pnts=3, dist_exponent=1.0)
    assert len(three.S) == len(plain.S) + 3 * (plain.frac_b == 0).sum()
    with pytest.raises(ValueError, match='points, the map'):
        weights.extrapolate(plain, src_ll[0][:-1], src_ll[1][:-1], *dst_ll,
                            'neareststod')


# ---------------------------------------------------------------------------
# 4. dispatch
# ---------------------------------------------------------------------------

def _grids():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return get_lat_lon_descriptor(10.0, 10.0), get_lat_lon_descriptor(6.0, 6.0)


def test_value_errors():
    from pyremap_amd import weights
    coarse, fine = _grids()
    for method in ('conserve', 'neareststod', 'conserve2nd'):
        with pytest.raises(ValueError, match="'bilinear', 'patch'"):
            weights.make_weights(coarse, fine, method,
                                 extrap_method='neareststod')
    for name in ('creep', 'nearestdtos', ''):
        with pytest.raises(ValueError,
                           match="'neareststod', 'nearestidavg'.*creep"):
            weights.make_weights(coarse, fine, 'bilinear', extrap_method=name)
    for n in (0, 17, -1, 2.5, True):
        with pytest.raises(ValueError, match='extrap_num_src_pnts'):
            weights.make_weights(coarse, fine, 'bilinear',
                                 extrap_method='nearestidavg',
                                 extrap_num_src_pnts=n)
    for p in (np.nan, np.inf, -0.5, 'two'):
        with pytest.raises(ValueError, match='extrap_dist_exponent'):
            weights.make_weights(coarse, fine, 'bilinear',
                                 extrap_method='nearestidavg',
                                 extrap_dist_exponent=p)
    for kw in ({'extrap_num_src_pnts': 4}, {'extrap_dist_exponent': 1.0}):
        with pytest.raises(ValueError, match='without extrap_method'):
            weights.make_weights(coarse, fine, 'bilinear', **kw)
        with pytest.raises(ValueError, match='without extrap_method'):
            weights.write_weights('unused.nc', coarse, fine, 'bilinear', **kw)
    # what stood before stands
    with pytest.raises(ValueError, match='expected one of'):
        weights.make_weights(coarse, fine, 'nope')
    assert weights.METHODS == ('conserve', 'bilinear', 'neareststod')


def test_neareststod_ignores_the_two_numbers(monkeypatch):
    from pyremap_amd import weights
    monkeypatch.setattr(weights, '_gpu_present', lambda: False)
    stereo, coarse = _stereo(), _grids()[0]
    a = weights.make_weights(stereo, coarse, 'bilinear',
                             extrap_method='neareststod')
    b = weights.make_weights(stereo, coarse, 'bilinear',
                             extrap_method='neareststod',
                             extrap_num_src_pnts=99,
                             extrap_dist_exponent=-3.0)
    for key in ('row', 'col', 'S', 'frac_b'):
        assert np.array_equal(getattr(a, key), getattr(b, key))


def test_without_extrap_method_every_call_is_the_one_made_before(monkeypatch):
    from pyremap_amd import weights
    calls = []
    for name in ('build_weights', 'bilinear_grid_weights', '_make_patch',
                 'extrapolate'):
        def fake(*args, _name=name, **kwargs):
            calls.append((_name, args, kwargs))
            return _name
        monkeypatch.setattr(weights, name, fake)
    coarse, fine = _grids()
    cells = qu240()
    for src, dst, method in ((coarse, fine, 'bilinear'),
                             (cells, coarse, 'bilinear'),
                             (cells, coarse, 'patch'),
                             (_stereo(), coarse, 'bilinear')):
        assert weights.make_weights(src, dst, method) in (
            'build_weights', '_make_patch')
        assert weights.make_weights(
            src, dst, method, extrap_method=None, extrap_num_src_pnts=None,
            extrap_dist_exponent=None) in ('build_weights', '_make_patch')
    assert len(calls) == 8 and 'extrapolate' not in {c[0] for c in calls}
    for name, args, kwargs in calls:
        assert kwargs == {}
        assert len(args) == (3 if name == 'build_weights' else 2)


def test_write_weights_passes_no_new_keyword(monkeypatch, tmp_path):
    from pyremap_amd import weights
    coarse, fine = _grids()
    plain = weights.build_weights(coarse, fine, 'bilinear')
    seen = []

    def fake(*args, **kwargs):
        seen.append((args, kwargs))
        return plain
    monkeypatch.setattr(weights, 'make_weights', fake)
    weights.write_weights(str(tmp_path / 'a.nc'), coarse, fine, 'bilinear')
    assert seen[-1] == ((coarse, fine, 'bilinear'), {})
    weights.write_weights(str(tmp_path / 'b.nc'), coarse, fine, 'bilinear',
                          extrap_method='nearestidavg')
    assert seen[-1] == ((coarse, fine, 'bilinear'),
                        {'extrap_method': 'nearestidavg'})
    weights.write_weights(str(tmp_path / 'c.nc'), coarse, fine, 'bilinear',
                          extrap_method='nearestidavg', extrap_num_src_pnts=4,
                          extrap_dist_exponent=1.5)
    assert seen[-1][1] == {'extrap_method': 'nearestidavg',
                           'extrap_num_src_pnts': 4,
                           'extrap_dist_exponent': 1.5}


def _global_attributes(path):
    from pyremap_amd.io.netcdf import open_dataset
    attrs = dict(open_dataset(path).attrs)
    return {k: (v.item() if isinstance(v, np.ndarray) and v.size == 1 else v)
            for k, v in attrs.items()}


NAMES = ('extrap_method', 'extrap_num_src_pnts', 'extrap_dist_exponent')


def test_file_attributes(monkeypatch, tmp_path):
    from pyremap_amd import weights
    from pyremap_amd.io import mapfile
    monkeypatch.setattr(weights, '_gpu_present', lambda: False)
    stereo, coarse = _stereo(), _grids()[0]
    path = str(tmp_path / 'plain.nc')
    plain = weights.write_weights(path, stereo, coarse, 'bilinear')
    attrs = _global_attributes(path)
    assert not any(name in attrs for name in NAMES)
    assert attrs['map_method'] == 'bilinear'
    for kw, want in (({'extrap_method': 'neareststod'}, ('neareststod', 1,
                                                         2.0)),
                     ({'extrap_method': 'nearestidavg'}, ('nearestidavg', 8,
                                                          2.0)),
                     ({'extrap_method': 'nearestidavg',
                       'extrap_num_src_pnts': 3,
                       'extrap_dist_exponent': 0.5}, ('nearestidavg', 3,
                                                      0.5))):
        path = str(tmp_path / f'map_{want[0]}_{want[1]}.nc')
        m = weights.write_weights(path, stereo, coarse, 'bilinear', **kw)
        attrs = _global_attributes(path)
        assert tuple(attrs[name] for name in NAMES) == want
        got = mapfile.read_mapping(path)
        assert np.array_equal(got.row, m.row) and np.array_equal(got.S, m.S)
        assert np.all(got.frac_b == 1.0)
        assert len(m.S) == len(plain.S) + want[1] * 548


def test_build_map_hands_the_attributes_on(monkeypatch, tmp_path):
    from pyremap_amd import Remapper, weights
    coarse, fine = _grids()
    plain = weights.build_weights(coarse, fine, 'bilinear')
    seen = []

    def fake(*args, **kwargs):
        seen.append((args, kwargs))
        return plain
    monkeypatch.setattr(weights, 'make_weights', fake)
    fresh = Remapper()
    assert fresh.extrap_method is None and fresh.extrap_num_src_pnts == 8
    assert fresh.extrap_dist_exponent == 2.0
    for method, n, p, want in (
            (None, 8, 2.0, {}),
            (None, 5, 1.0, {}),
            ('neareststod', 5, 1.0, {'extrap_method': 'neareststod'}),
            ('nearestidavg', 8, 2.0, {'extrap_method': 'nearestidavg',
                                      'extrap_num_src_pnts': 8,
                                      'extrap_dist_exponent': 2.0}),
            ('nearestidavg', 5, 1.0, {'extrap_method': 'nearestidavg',
                                      'extrap_num_src_pnts': 5,
                                      'extrap_dist_exponent': 1.0})):
        r = Remapper(ntasks=1, method='bilinear', map_tool='analytic',
                     use_tmp=False, src_descriptor=coarse,
                     dst_descriptor=fine,
                     map_filename=str(tmp_path / f'map_{len(seen)}.nc'))
        r.extrap_method, r.extrap_num_src_pnts = method, n
        r.extrap_dist_exponent = p
        r.build_map()
        args, kwargs = seen[-1]
        assert args == (coarse, fine, 'bilinear')
        assert kwargs == want
        attrs = _global_attributes(r.map_filename)
        assert ('extrap_method' in attrs) == (method is not None)
    for word in NAMES:
        assert word in Remapper.build_map.__doc__


# ---------------------------------------------------------------------------
# 5. ABI
# ---------------------------------------------------------------------------

def test_abi_names():
    from pyremap_amd import _build, engine, weights
    names = ('remap_nearest_k_workspace', 'remap_nearest_k')
    header = open(os.path.join(REPO, 'include', 'remap_hip.h')).read()
    script = open(os.path.join(REPO, 'pyremap_amd', 'csrc',
                               'libremap_hip.map')).read()
    exported = re.search(r'global:(.*?)local:', script, re.S).group(1)
    patterns = [p.strip() for p in exported.split(';') if p.strip()]
    assert 'remap_nearest.hip' in _build.SOURCES
    for name in names:
        assert name in engine.EXPORTS
        assert re.search(r'REMAP_API\s+int ' + name + r'\(', header)
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns)
        assert hasattr(engine.load_library(), name)
    assert re.search(r'#define REMAP_NEAREST_K_MAX 16\b', header)
    assert engine.NEAREST_K_MAX == weights.NEAREST_K_MAX == 16
    assert engine.ABI_VERSION == 31
    assert re.search(r'#define REMAP_ABI_VERSION 31\b', header)
    assert callable(engine.nearest_k_points)


def test_the_engine_call_needs_the_gpu(monkeypatch):
    import torch
    from pyremap_amd import engine
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    x = torch.zeros((4, 3), dtype=torch.float64)
    with pytest.raises(engine.EngineError, match='no HIP device'):
        engine.nearest_k_points(x, x, 2)
