"""
Record dimensions in NetCDF-4 output: the chunked, deflated storage of
pyremap_amd/io/hdf5_write.py (version-1 chunk B-trees, shuffle + deflate,
unlimited maxima), the encoding keys that carry it through ``open_dataset``
/ ``write_netcdf``, and the extensible-array chunk index
pyremap_amd/io/hdf5_lite.py reads from ``libver='latest'`` files
(tests/golden/make_record_fixtures.py -> tests/golden/hdf5/records.h5,
expected_records.npz).  CPU only.
"""
import hashlib
import json
import os
import subprocess
from collections import OrderedDict

import numpy as np
import pytest

from pyremap_amd.io import hdf5_lite, hdf5_write, netcdf
from pyremap_amd.io.hdf5_write import write_netcdf4
from pyremap_amd.io.netcdf4_lite import NetCDF4File
from pyremap_amd.xr_lite import LazyValues

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, 'golden', 'hdf5')
K = hdf5_write.CHUNK_BTREE_K
UNLIMITED = (1 << 64) - 1


def _layout(dataset):
    """(class, chunk shape, B-tree address) of a version-3 layout message."""
    f = dataset.file
    pos, _ = dataset._find(hdf5_lite.MSG_LAYOUT)
    assert f.mm[pos] == 3
    cls = f.mm[pos + 1]
    if cls != 2:
        return cls, None, None
    rank = f.mm[pos + 2] - 1
    chunks = tuple(f.uint(pos + 3 + f.O + 4 * i, 4) for i in range(rank))
    return cls, chunks, f.addr(pos + 3)


def _tree_depth(dataset):
    """Levels of the chunk B-tree, read from its root node."""
    f = dataset.file
    tree = _layout(dataset)[2]
    assert f.mm[tree:tree + 4] == b'TREE' and f.mm[tree + 4] == 1
    return f.mm[tree + 5] + 1


def _round_trip_variables():
    """The variable set of test_hdf5_cpu.test_netcdf4_writer_round_trip."""
    rng = np.random.default_rng(0)
    dims = OrderedDict([('time', 2), ('lat', 3), ('lon', 4), ('nchar', 5),
                        ('big', 300)])
    label = np.array([list(b'hello'), list(b'world')],
                     dtype='u1').view('S1').reshape(2, 5)
    variables = [
        ('lat', ('lat',), np.linspace(-60, 60, 3), {'units': 'degrees_north'}),
        ('lon', ('lon',), np.linspace(0, 270, 4).astype('>f8'), {}),
        ('temp', ('time', 'lat', 'lon'),
         rng.standard_normal((2, 3, 4)).astype('f4'),
         {'units': 'K', '_FillValue': np.float32(9.96921e36),
          'valid_range': np.array([-5.0, 5.0], 'f4'),
          'flag_values': np.array([1, 2, 3], 'i1')}),
        ('count', ('time',), np.array([3, 4], 'i4'), {}),
        ('wide', ('big', 'lon'), rng.integers(0, 1 << 40, (300, 4)), {}),
        ('u16', ('lat',), np.array([1, 2, 65535], 'u2'), {}),
        ('scalar', (), np.float64(2.5), {'long_name': 'a scalar variable'}),
        ('zeros', ('time', 'lat'), np.zeros((2, 3)), {}),
        ('label', ('time', 'nchar'), label, {}),
    ]
    for i in range(60):
        variables.append((f'v{i:02d}', ('lat',), rng.random(3), {}))
    attrs = OrderedDict([('title', 'written here'),
                         ('history', 'line 1\nline 2'),
                         ('version', np.int32(3)),
                         ('scale', 0.5), ('levels', [1, 2, 3])])
    return dims, variables, attrs


def test_record_dimension_round_trip(tmp_path):
    """``unlimited=['time']``: the dimension reads back unlimited; names,
    dtypes, values and attributes as written; every dataset along ``time``
    -- its placeholder scale too -- is chunked with extent 1 on that axis
    and an unlimited maximum there, every other one still contiguous."""
    dims, variables, attrs = _round_trip_variables()
    path = str(tmp_path / 'records.nc')
    write_netcdf4(path, dims, variables, attrs=attrs, unlimited=['time'])
    with NetCDF4File(path) as nc:
        assert nc.unlimited == ['time']
        assert list(nc.dimensions.items()) == list(dims.items())
        for name, vdims, data, vattrs in variables:
            var = nc.variables[name]
            assert var.dims == tuple(vdims), name
            got, want = var.read(), np.asarray(data)
            assert got.dtype == want.dtype.newbyteorder('='), name
            np.testing.assert_array_equal(got, want, err_msg=name)
            assert sorted(var.attrs) == sorted(vattrs), name
            for k, v in vattrs.items():
                np.testing.assert_array_equal(np.asarray(var.attrs[k]),
                                              np.asarray(v), err_msg=k)
        assert nc.attrs['title'] == 'written here'
        assert nc.attrs['history'] == 'line 1\nline 2'
        assert np.asarray(nc.attrs['levels']).tolist() == [1, 2, 3]
    along = {name: vdims for name, vdims, _, _ in variables}
    along.update({'time': ('time',), 'nchar': ('nchar',), 'big': ('big',)})
    with hdf5_lite.File(path) as f:
        assert sorted(f.root.keys()) == sorted(along)
        for name, vdims in along.items():
            d = f.root[name]
            cls, chunks, tree = _layout(d)
            if 'time' not in vdims:
                assert cls == 1 and d.maxshape is None, name
                continue
            assert cls == 2, name
            axis = vdims.index('time')
            assert chunks[axis] == 1, (name, chunks)
            assert chunks == tuple(1 if i == axis else n
                                   for i, n in enumerate(d.shape)), name
            assert d.maxshape == tuple(UNLIMITED if i == axis else n
                                       for i, n in enumerate(d.shape)), name
            # the placeholder owns no chunk
            assert (tree is None) == (name == 'time'), name


@pytest.mark.parametrize('records, depth', [(1, 1), (2 * K, 1),
                                            (2 * K + 1, 2),
                                            ((2 * K) ** 2 + 1, 3)])
def test_chunk_btree_levels(tmp_path, records, depth):
    """One chunk per record: one node, a full node, two levels, three --
    every value back, the depth as read from the file's root node."""
    data = np.arange(records * 3, dtype='i4').reshape(records, 3) * 7 - 5
    path = str(tmp_path / 'levels.nc')
    write_netcdf4(path, OrderedDict([('n', records), ('c', 3)]),
                  [('v', ('n', 'c'), data, {})], unlimited=['n'])
    with hdf5_lite.File(path) as f:
        d = f.root['v']
        assert _layout(d)[1] == (1, 3)
        assert _tree_depth(d) == depth
        np.testing.assert_array_equal(d.read(), data)
    with NetCDF4File(path) as nc:
        assert nc.unlimited == ['n'] and nc.dimensions['n'] == records


def test_zero_records(tmp_path):
    path = str(tmp_path / 'empty.nc')
    write_netcdf4(path, OrderedDict([('t', 0), ('x', 4)]),
                  [('v', ('t', 'x'), np.zeros((0, 4), 'f4'), {}),
                   ('z', ('t', 'x'), np.zeros((0, 4)), {})],
                  unlimited=['t'], encoding={'z': {'zlib': True}})
    with NetCDF4File(path) as nc:
        assert nc.unlimited == ['t']
        assert dict(nc.dimensions) == {'t': 0, 'x': 4}
        for name, dtype in (('v', 'f4'), ('z', 'f8')):
            got = nc.variables[name].read()
            assert got.shape == (0, 4) and got.dtype == np.dtype(dtype)
    with hdf5_lite.File(path) as f:
        for name in ('v', 'z', 't'):
            cls, chunks, tree = _layout(f.root[name])
            assert cls == 2 and tree is None, name
            assert f.root[name].maxshape[0] == UNLIMITED
        assert _layout(f.root['v'])[1] == (1, 4)


def test_default_chunks_are_split_below_the_byte_limit(tmp_path, monkeypatch):
    """CHUNK_BYTES_MAX = 64: a (3, 7, 5) float64 variable along an unlimited
    first axis starts from (1, 7, 5) = 280 bytes; halving the fixed axes in
    turn, ceiling division: (1, 4, 5) = 160, (1, 4, 3) = 96, (1, 2, 3) = 48.
    Both split axes end on a ragged chunk: 7 = 3 * 2 + 1, 5 = 3 + 2."""
    assert 0 < hdf5_write.CHUNK_BYTES_MAX < 1 << 32
    monkeypatch.setattr(hdf5_write, 'CHUNK_BYTES_MAX', 64)
    assert hdf5_write.default_chunks((3, 7, 5), (True, False, False), 8) == \
        (1, 2, 3)
    # exactly at the limit is not under it; nothing left to halve ends it
    assert hdf5_write.default_chunks((3, 8), (True, False), 8) == (1, 4)
    assert hdf5_write.default_chunks((3, 2), (True, False), 128) == (1, 1)
    data = np.random.default_rng(1).standard_normal((3, 7, 5))
    path = str(tmp_path / 'split.nc')
    write_netcdf4(path, OrderedDict([('t', 3), ('y', 7), ('x', 5)]),
                  [('v', ('t', 'y', 'x'), data, {})], unlimited=['t'])
    with hdf5_lite.File(path) as f:
        d = f.root['v']
        assert _layout(d)[1] == (1, 2, 3)
        chunks = []
        d._chunks_btree1(_layout(d)[2], 3, chunks)
        assert len(chunks) == 3 * 4 * 2
        assert all(size == 48 for _, _, size, _ in chunks)
        assert {o[1] for o, _, _, _ in chunks} == {0, 2, 4, 6}
        assert {o[2] for o, _, _, _ in chunks} == {0, 3}
        got = d.read()
    np.testing.assert_array_equal(got, data)
    np.testing.assert_array_equal(got[:, 6:, :], data[:, 6:, :])   # ragged y
    np.testing.assert_array_equal(got[:, :, 3:], data[:, :, 3:])   # ragged x


def _deferred(array, log=None):
    def load():
        if log is not None:
            log.append(array.shape)
        return array.copy()
    return LazyValues(array.shape, array.dtype, load)


@pytest.mark.parametrize('shuffle', [False, True])
@pytest.mark.parametrize('level', [1, 9])
def test_filters(tmp_path, level, shuffle):
    """Deflate at both ends of its range, with and without shuffle, on
    float32 / float64 / int16 / S1 data; NaN -> fill before the filters for
    a known array (``nan_fill``) and for arrays produced on demand
    (``auto_fill``, with and without NaNs); a filtered variable with no
    unlimited dimension.  Values equal, the encoding ``open_dataset``
    reports is the one asked for, constant data shrinks."""
    rng = np.random.default_rng(level * 2 + shuffle)
    f32 = rng.standard_normal((5, 6, 7)).astype('f4')
    f32[1, 2, 3] = f32[4, 5, 6] = np.nan
    f64 = rng.standard_normal((5, 6, 7))
    holed = f64.copy()
    holed[0, :, 2] = np.nan
    i16 = rng.integers(-30000, 30000, (5, 7)).astype('i2')
    text = rng.integers(65, 91, (5, 9)).astype('u1').view('S1')
    fixed = rng.standard_normal((6, 7))
    const = np.full((5, 6, 7), 2.5)
    fill32, fill64 = np.float32(9.96921e36), np.float64(9.969209968386869e36)
    dims = OrderedDict([('t', 5), ('y', 6), ('x', 7), ('c', 9)])
    loaded = []

    def variables():
        return [('f32', ('t', 'y', 'x'), f32, {'_FillValue': fill32}),
                ('clean', ('t', 'y', 'x'), _deferred(f64, loaded), {}),
                ('holed', ('t', 'y', 'x'), _deferred(holed, loaded), {}),
                ('i16', ('t', 'x'), i16, {'units': 'counts'}),
                ('text', ('t', 'c'), text, {}),
                ('fixed', ('y', 'x'), fixed, {}),
                ('const', ('t', 'y', 'x'), const, {}),
                ('scalar', (), np.float64(1.0), {})]
    asked = {'zlib': True, 'complevel': level, 'shuffle': shuffle}
    names = [v[0] for v in variables()]
    path, twin = str(tmp_path / 'packed.nc'), str(tmp_path / 'plain.nc')
    kw = dict(unlimited=['t'], nan_fill={'f32': fill32},
              auto_fill={'clean': fill64, 'holed': fill64})
    write_netcdf4(path, dims, variables(),
                  encoding={n: asked for n in names}, **kw)
    write_netcdf4(twin, dims, variables(), **kw)
    assert sorted(loaded) == sorted([f64.shape] * 4)       # once per write
    sizes = []
    for enc in ({'const': asked}, None):
        alone = str(tmp_path / 'const.nc')
        write_netcdf4(alone, dims, [variables()[-2]], unlimited=['t'],
                      encoding=enc)
        sizes.append(os.path.getsize(alone))
    assert sizes[0] < sizes[1]
    vdims = {v[0]: v[1] for v in variables()}
    want = {'f32': np.where(np.isnan(f32), fill32, f32), 'clean': f64,
            'holed': np.where(np.isnan(holed), fill64, holed), 'i16': i16,
            'text': text, 'fixed': fixed, 'const': const,
            'scalar': np.float64(1.0)}
    for file, filtered in ((path, True), (twin, False)):
        raw = netcdf.open_dataset(file, mask_and_scale=False)
        assert raw.encoding['unlimited_dims'] == ['t']
        for name in names:
            var = raw.variables[name]
            assert var.values.dtype == want[name].dtype, name
            np.testing.assert_array_equal(var.values, want[name],
                                          err_msg=name)
            enc = var.encoding
            along_t = name not in ('fixed', 'scalar')
            if name == 'scalar' or not (filtered or along_t):
                assert enc['contiguous'] and enc['chunksizes'] is None, name
            else:
                assert not enc['contiguous'], name
                assert enc['chunksizes'] == tuple(
                    1 if d == 't' else dims[d] for d in vdims[name]), name
            if filtered and name != 'scalar':
                assert {k: enc[k] for k in asked} == asked, name
            else:
                assert (enc['zlib'], enc['complevel'], enc['shuffle']) == \
                    (False, 0, False), name
        # _FillValue only where NaNs turned up
        assert raw.variables['holed'].attrs['_FillValue'] == fill64
        assert '_FillValue' not in raw.variables['clean'].attrs
    back = netcdf.open_dataset(path)
    np.testing.assert_array_equal(back['holed'].values, holed)   # NaNs back
    np.testing.assert_array_equal(back['f32'].values, f32)


def test_explicit_chunk_shape_and_bad_encodings(tmp_path):
    data = np.arange(70.0).reshape(7, 10)
    path = str(tmp_path / 'given.nc')
    dims = OrderedDict([('y', 7), ('x', 10)])
    write_netcdf4(path, dims, [('v', ('y', 'x'), data, {})],
                  encoding={'v': {'chunksizes': (3, 4)}})
    raw = netcdf.open_dataset(path, mask_and_scale=False)
    enc = raw.variables['v'].encoding
    assert enc['chunksizes'] == (3, 4) and not enc['zlib']
    np.testing.assert_array_equal(raw['v'].values, data)
    for bad, match in (({'w': {'zlib': True}}, 'no such variables'),
                       ({'v': {'gzip': 4}}, 'unknown encoding keys'),
                       ({'v': {'chunksizes': (3,)}}, 'do not fit'),
                       ({'v': {'chunksizes': (8, 4)}}, 'do not fit'),
                       ({'v': {'chunksizes': (0, 4)}}, 'do not fit'),
                       ({'v': {'zlib': True, 'complevel': 12}}, 'zlib level')):
        with pytest.raises(ValueError, match=match):
            write_netcdf4(path, dims, [('v', ('y', 'x'), data, {})],
                          encoding=bad)


#: sha256 of the file the snippet in test_default_output_is_unchanged writes,
#: computed with the writer as it was before it learnt chunked storage
PARENT_SHA256 = \
    '24feaaa93a9ed842ad824b8978746d56da0d3d40303dc93df96e08a61f143047'


def test_default_output_is_unchanged(tmp_path):
    """Without ``unlimited`` and without filters the writer produces, byte
    for byte, the contiguous file it produced before chunked storage
    existed.  ``PARENT_SHA256`` is what this snippet printed on the commit
    before::

        write_netcdf4(
            path, OrderedDict([('time', 2), ('y', 3), ('x', 4)]),
            [('x', ('x',), np.arange(4.0), {'units': 'm'}),
             ('t', ('time', 'y', 'x'),
              np.arange(24, dtype='f4').reshape(2, 3, 4),
              {'long_name': 'field'}),
             ('n', ('time',), np.array([7, 8], 'i4'), {}),
             ('s', (), np.float64(1.5), {})],
            attrs={'title': 'unchanged'})
        print(hashlib.sha256(open(path, 'rb').read()).hexdigest())
    """
    path = str(tmp_path / 'default.nc')
    write_netcdf4(
        path, OrderedDict([('time', 2), ('y', 3), ('x', 4)]),
        [('x', ('x',), np.arange(4.0), {'units': 'm'}),
         ('t', ('time', 'y', 'x'),
          np.arange(24, dtype='f4').reshape(2, 3, 4),
          {'long_name': 'field'}),
         ('n', ('time',), np.array([7, 8], 'i4'), {}),
         ('s', (), np.float64(1.5), {})],
        attrs={'title': 'unchanged'})
    assert hashlib.sha256(open(path, 'rb').read()).hexdigest() == \
        PARENT_SHA256


def test_write_netcdf_encoding(tmp_path):
    """``write_netcdf(..., encoding=...)``: NetCDF-4 only; what a Dataset
    remembers of the file it came from is NOT applied by default."""
    import pyremap_amd
    ds = pyremap_amd.Dataset()
    t = np.arange(24.0).reshape(2, 3, 4)
    t[1, 2, 3] = np.nan
    ds['t'] = pyremap_amd.DataArray(t, dims=('Time', 'y', 'x'))
    ds['n'] = pyremap_amd.DataArray(np.array([1, 2], 'i4'), dims=('Time',))
    asked = {'t': {'zlib': True, 'complevel': 5, 'shuffle': True},
             'n': {'zlib': True, 'complevel': 2, 'shuffle': False}}
    for fmt in ('NETCDF3_CLASSIC', 'NETCDF3_64BIT', 'NETCDF3_64BIT_DATA'):
        with pytest.raises(ValueError, match='NetCDF-4'):
            netcdf.write_netcdf(ds, str(tmp_path / 'c.nc'), format=fmt,
                                encoding=asked)
        netcdf.write_netcdf(ds, str(tmp_path / 'c.nc'), format=fmt,
                            encoding={})                  # empty: harmless
    packed = str(tmp_path / 'packed.nc')
    netcdf.write_netcdf(ds, packed, format='NETCDF4',
                        unlimited_dims=['Time'], encoding=asked)
    back = netcdf.open_dataset(packed)
    assert back.encoding['unlimited_dims'] == ['Time']
    for name, enc in asked.items():
        got = back.variables[name].encoding
        assert {k: got[k] for k in enc} == enc, name
        assert not got['contiguous']
    assert back.variables['t'].encoding['chunksizes'] == (1, 3, 4)
    assert back.variables['t'].encoding['_FillValue'] == \
        9.969209968386869e+36                             # the old key stays
    np.testing.assert_array_equal(back['t'].values, t)
    again = str(tmp_path / 'again.nc')
    netcdf.write_netcdf(back, again, format='NETCDF4')     # encoding=None
    plain = netcdf.open_dataset(again)
    assert plain.encoding['unlimited_dims'] == ['Time']
    for name in asked:
        got = plain.variables[name].encoding
        assert (got['zlib'], got['complevel'], got['shuffle']) == \
            (False, 0, False), name
        assert not got['contiguous']          # the record dimension chunks
    np.testing.assert_array_equal(plain['t'].values, t)
    assert os.path.getsize(again) != os.path.getsize(packed)


# ---------------------------------------------------------------------------
# reader: the extensible-array chunk index of libver='latest' files
# ---------------------------------------------------------------------------

@pytest.fixture(scope='module')
def expected_records():
    return np.load(os.path.join(GOLDEN, 'expected_records.npz'))


@pytest.mark.parametrize('records', [1, 4, 5, 40, 3000])
@pytest.mark.parametrize('kind', ['plain', 'packed'])
def test_extensible_array_index(expected_records, kind, records):
    """1 and 4 records: the index block's own elements; 5 and 40: data
    blocks addressed from the index block; 3000: data blocks addressed from
    super blocks (make_record_fixtures.py says how that was confirmed).
    Unfiltered float64 and gzip 4 + shuffle float32, chunks of one record."""
    name = f'{kind}_{records}'
    with hdf5_lite.File(os.path.join(GOLDEN, 'records.h5')) as f:
        d = f.root[name]
        pos, _ = d._find(hdf5_lite.MSG_LAYOUT)
        assert f.mm[pos] == 4 and f.mm[pos + 1] == 2      # version 4, chunked
        assert d.maxshape[0] == UNLIMITED
        got = d.read()
        store = d.storage()
    want = expected_records[f'records:{name}']
    assert got.dtype == want.dtype and got.shape == (records, want.shape[1])
    np.testing.assert_array_equal(got, want)
    assert store['chunks'] == (1, want.shape[1])
    assert store['filters'] == ([(2, [4]), (1, [4])] if kind == 'packed'
                                else [])


def test_extensible_array_along_a_later_axis(expected_records):
    """The unlimited axis is the array's slowest one wherever it stands."""
    with hdf5_lite.File(os.path.join(GOLDEN, 'records.h5')) as f:
        got = f.root['sideways'].read()
    np.testing.assert_array_equal(got, expected_records['records:sideways'])
    assert got.shape == (4, 7)


def test_unread_chunk_indexes_are_named():
    with hdf5_lite.File(os.path.join(GOLDEN, 'records.h5')) as f:
        with pytest.raises(NotImplementedError,
                           match='v2 B-tree.*two_axes'):
            f.root['two_axes'].read()


def test_extensible_array_signatures_are_checked(tmp_path):
    """A damaged block is reported, not read through."""
    raw = open(os.path.join(GOLDEN, 'records.h5'), 'rb').read()
    for signature, what in ((b'EAHD', 'header'), (b'EAIB', 'index block'),
                            (b'EADB', 'data block'),
                            (b'EASB', 'super block')):
        path = str(tmp_path / f'{signature.decode()}.h5')
        with open(path, 'wb') as out:
            out.write(raw.replace(signature, b'XXXX'))
        with hdf5_lite.File(path) as f:
            with pytest.raises(ValueError,
                               match=f'extensible array {what} signature'):
                f.root['packed_3000'].read()


def test_record_fixture_opens_as_a_dataset(expected_records):
    """The netCDF-4 shaped fixture (the GPU test's second input writer)."""
    ds = netcdf.open_dataset(os.path.join(GOLDEN, 'record_input.nc'))
    assert ds.encoding['unlimited_dims'] == ['Time']
    np.testing.assert_array_equal(ds['field'].values,
                                  expected_records['record_input:field'])
    for name, chunks in (('field', (1, 6, 12)), ('count', (1,)),
                         ('xtime', (1, 10))):
        enc = ds.variables[name].encoding
        assert (enc['zlib'], enc['complevel'], enc['shuffle'],
                enc['chunksizes'], enc['contiguous']) == \
            (True, 4, True, chunks, False), name


# ---------------------------------------------------------------------------
# cross-check against libhdf5
# ---------------------------------------------------------------------------

H5PY_PYTHON = '/opt/conda/bin/python3.9'


def _h5py_python():
    if not os.path.exists(H5PY_PYTHON):
        return None
    try:
        done = subprocess.run([H5PY_PYTHON, '-c', 'import h5py, numpy'],
                              capture_output=True)
    except OSError:
        return None
    return H5PY_PYTHON if done.returncode == 0 else None


def test_libhdf5_reads_the_chunked_files(tmp_path):
    """h5py (libhdf5) on files from this writer: values, ``maxshape``,
    chunk shapes, gzip level, shuffle, dimension scales -- see
    tests/check_records_h5py.py.  One file covers a three-level B-tree, a
    split chunk shape with ragged edges, every filter combination, a
    deferred variable, a filtered variable without a record dimension and a
    scalar; a second one zero records."""
    python = _h5py_python()
    if python is None:
        pytest.skip(f'{H5PY_PYTHON} with h5py is not on this machine')
    rng = np.random.default_rng(3)
    n = (2 * K) ** 2 + 1
    holed = rng.standard_normal((4, 7, 5))
    holed[2, 3, :] = np.nan
    fill = np.float64(9.969209968386869e36)
    text = rng.integers(65, 91, (4, 9)).astype('u1').view('S1')
    cases = {
        'many': [OrderedDict([('n', n), ('c', 3), ('time', 4), ('y', 7),
                              ('x', 5), ('len', 9)]),
                 [('many', ('n', 'c'),
                   np.arange(n * 3, dtype='i4').reshape(n, 3), {}),
                  ('n', ('n',), np.arange(n, dtype='f8'), {}),
                  ('holed', ('time', 'y', 'x'), _deferred(holed), {}),
                  ('split', ('time', 'y', 'x'),
                   rng.standard_normal((4, 7, 5)).astype('f4'), {}),
                  ('shuffled', ('time', 'x'),
                   rng.integers(-9, 9, (4, 5)).astype('i2'), {}),
                  ('text', ('time', 'len'), text, {}),
                  ('static', ('y', 'x'), rng.standard_normal((7, 5)), {}),
                  ('loose', ('y',), np.arange(7, dtype='i4'), {}),
                  ('scalar', (), np.float64(2.5), {})],
                 ['n', 'time'],
                 {'holed': {'zlib': True, 'complevel': 1, 'shuffle': True},
                  'split': {'zlib': True, 'complevel': 9, 'shuffle': False,
                            'chunksizes': (1, 4, 3)},
                  'shuffled': {'shuffle': True},
                  'text': {'zlib': True, 'complevel': 4, 'shuffle': True},
                  'static': {'zlib': True, 'complevel': 6}}],
        'empty': [OrderedDict([('time', 0), ('x', 5)]),
                  [('v', ('time', 'x'), np.zeros((0, 5), 'f4'), {}),
                   ('x', ('x',), np.arange(5.0), {})],
                  ['time'], {'v': {'zlib': True, 'complevel': 3}}],
    }
    for tag, (dims, variables, unlimited, encoding) in cases.items():
        path = str(tmp_path / f'{tag}.nc')
        write_netcdf4(path, dims, variables, unlimited=unlimited,
                      auto_fill={'holed': fill}, encoding=encoding)
        payload, storage = {}, {}
        for name, vdims, data, _ in variables:
            payload[f'var/{name}'] = np.where(np.isnan(holed), fill, holed) \
                if name == 'holed' else np.asarray(data)
            enc = encoding.get(name, {})
            chunked = bool(vdims) and (bool(enc) or
                                       any(d in unlimited for d in vdims))
            storage[name] = {
                'chunks': list(enc.get('chunksizes') or
                               [1 if d in unlimited else max(dims[d], 1)
                                for d in vdims]) if chunked else None,
                'complevel': enc.get('complevel', 0) if enc.get('zlib')
                else 0,
                'shuffle': bool(enc.get('shuffle'))}
        payload['__meta__'] = np.array(json.dumps({
            'dimensions': dims, 'unlimited': unlimited,
            'variables': {v[0]: list(v[1]) for v in variables},
            'storage': storage}))
        npz = str(tmp_path / f'{tag}.npz')
        np.savez(npz, **payload)
        done = subprocess.run(
            [python, os.path.join(HERE, 'check_records_h5py.py'), path, npz],
            capture_output=True, text=True,
            env={k: v for k, v in os.environ.items()
                 if not k.startswith('PYTHON')})
        assert done.returncode == 0, done.stdout + done.stderr
        assert done.stdout.startswith('OK ')
