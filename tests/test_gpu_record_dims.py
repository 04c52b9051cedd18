"""
GPU test of the file -> GPU -> file path on NetCDF-4 input with a record
dimension: ``Remapper.ncremap`` keeps ``Time`` unlimited and every variable's
deflate level and shuffle flag, whichever writer made the input -- this
package's (v1 B-tree chunk index) or h5py with ``libver='latest'``
(extensible array; tests/golden/make_record_fixtures.py ->
tests/golden/hdf5/record_input.nc) -- eagerly and streamed.
"""
import os

import numpy as np
import pytest

from helpers import assert_bitwise

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'hdf5')
PACKED = {'zlib': True, 'complevel': 4, 'shuffle': True}
NAMES = ('field', 'count', 'xtime')


def record_field():
    """make_record_fixtures.record_field: (3, 6, 12) float64 with NaNs."""
    t, i, j = np.meshgrid(np.arange(3.0), np.arange(6.0), np.arange(12.0),
                          indexing='ij')
    field = np.sin(0.5 * i) * np.cos(0.25 * j) + 0.125 * t
    field[(t + i + j) % 7 == 0] = np.nan
    field[1, :2, :4] = np.nan          # whole destination cells go missing
    return field


def input_dataset():
    from pyremap_amd import DataArray, Dataset
    ds = Dataset(attrs={'title': 'record fixture'})
    ds['field'] = DataArray(record_field(), dims=('Time', 'lat', 'lon'),
                            attrs={'units': 'K'})
    ds['count'] = DataArray(np.array([10, 20, 30], 'i4'), dims=('Time',))
    ds['xtime'] = DataArray(
        np.frombuffer(b'0001-01-010001-02-010001-03-01',
                      dtype='S1').reshape(3, 10), dims=('Time', 'StrLen'))
    return ds


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    assert torch.cuda.is_available()
    from pyremap_amd import Remapper, get_lat_lon_descriptor
    from pyremap_amd.io.netcdf import write_netcdf
    tmp = tmp_path_factory.mktemp('records')
    src = get_lat_lon_descriptor(30.0, 30.0)
    dst = get_lat_lon_descriptor(45.0, 45.0)
    map_path = str(tmp / 'map_30deg_to_45deg_conserve.nc')
    r = Remapper(map_filename=map_path, method='conserve',
                 map_tool='analytic', src_descriptor=src, dst_descriptor=dst)
    r.build_map()
    ours = str(tmp / 'in_ours.nc')
    write_netcdf(input_dataset(), ours, format='NETCDF4',
                 unlimited_dims=['Time'],
                 encoding={name: PACKED for name in NAMES})
    inputs = {'ours': ours, 'h5py': os.path.join(GOLDEN, 'record_input.nc')}

    def remapper():
        return Remapper(map_filename=map_path, method='conserve',
                        src_descriptor=src, dst_descriptor=dst)
    return dict(tmp=tmp, inputs=inputs, remapper=remapper)


def _check_output(path, ref, source):
    from pyremap_amd.io.netcdf import file_format, open_dataset
    assert file_format(path) == 'NETCDF4'
    out = open_dataset(path)
    assert out.encoding['unlimited_dims'] == ['Time']
    # (the writer's group lists its members by name, whatever their order
    # in the input)
    assert sorted(out.data_vars) == sorted(ref.data_vars) == sorted(NAMES)
    for name in NAMES:
        enc = out.variables[name].encoding
        assert {k: enc[k] for k in PACKED} == PACKED, name
        assert not enc['contiguous'] and enc['chunksizes'][0] == 1, name
    for name in ('lat', 'lon'):             # new: no input variable to copy
        enc = out.variables[name].encoding
        assert enc['contiguous'] and not enc['zlib'] and not enc['shuffle']
    assert out['field'].dims == ('Time', 'lat', 'lon')
    assert out['field'].shape == (3, 4, 8)
    assert_bitwise(out['field'].values, ref['field'].values, 'field')
    assert np.isnan(out['field'].values).any()
    np.testing.assert_array_equal(out['count'].values, source['count'].values)
    assert out['count'].dtype == np.int32
    assert out['xtime'].values.tobytes() == source['xtime'].values.tobytes()
    return out


@pytest.mark.parametrize('writer', ['ours', 'h5py'])
def test_ncremap_keeps_record_dimension_and_filters(setup, writer,
                                                    monkeypatch):
    from pyremap_amd.io.netcdf import open_dataset
    from pyremap_amd.remapper import remap_file
    src_path = setup['inputs'][writer]
    source = open_dataset(src_path)
    assert source.encoding['unlimited_dims'] == ['Time']
    want = input_dataset()
    np.testing.assert_array_equal(source['field'].values,
                                  want['field'].values)     # the same content
    for name in NAMES:
        enc = source.variables[name].encoding
        assert {k: enc[k] for k in PACKED} == PACKED, name
    r = setup['remapper']()
    ref = r.remap_numpy(open_dataset(src_path),
                        renormalization_threshold=0.01)
    eager = str(setup['tmp'] / f'out_{writer}.nc')
    r.ncremap(src_path, eager, renormalize=0.01)
    a = _check_output(eager, ref, source)
    # every variable through the deferred path: the same file contents
    monkeypatch.setattr(remap_file, 'STREAM_BYTES', 1)
    streamed = str(setup['tmp'] / f'out_{writer}_streamed.nc')
    setup['remapper']().ncremap(src_path, streamed, renormalize=0.01)
    b = _check_output(streamed, ref, source)
    raw_a = open_dataset(eager, mask_and_scale=False)
    raw_b = open_dataset(streamed, mask_and_scale=False)
    assert list(raw_a.variables) == list(raw_b.variables)
    for name in raw_a.variables:
        va, vb = raw_a.variables[name], raw_b.variables[name]
        assert va.dims == vb.dims and va.dtype == vb.dtype, name
        assert va.values.tobytes() == vb.values.tobytes(), name
        assert sorted(va.attrs) == sorted(vb.attrs), name
        assert a.variables[name].encoding == b.variables[name].encoding, name


def test_ncremap_netcdf3_input_stays_netcdf3(setup):
    from pyremap_amd.io.netcdf import file_format, open_dataset, write_netcdf
    src_path = str(setup['tmp'] / 'in_classic.nc')
    write_netcdf(input_dataset(), src_path, format='NETCDF3_64BIT_DATA',
                 unlimited_dims=['Time'])
    out_path = str(setup['tmp'] / 'out_classic.nc')
    setup['remapper']().ncremap(src_path, out_path, renormalize=0.01)
    assert file_format(out_path) == 'NETCDF3_64BIT_DATA'
    assert open_dataset(out_path).encoding['unlimited_dims'] == ['Time']
