#!/opt/conda/bin/python3.9
"""
HDF5 files with record (unlimited) dimensions as h5py writes them with
``libver='latest'``: chunked datasets indexed by an EXTENSIBLE ARRAY (data
layout version 4, chunk index type 4), which pyremap_amd/io/hdf5_lite.py
reads.  Written with h5py (the image's conda interpreter has it; the
interpreter the package runs on does not); ``expected_records.npz`` holds
every dataset as h5py reads it back.

    /opt/conda/bin/python3.9 tests/golden/make_record_fixtures.py

``records.h5``: for n = 1, 4, 5, 40 and 3000 records a float64 dataset
``plain_<n>`` (n, 3), unfiltered, and a float32 dataset ``packed_<n>``
(n, 4), gzip 4 + shuffle, both with one unlimited axis and chunks of one
record.  With libhdf5's parameters for this index (4 elements in the index
block, data blocks of at least 16 elements, 4 data-block pointers in the
smallest super block) the array's elements sit, as read from the files'
structures (the EAIB / EADB / EASB blocks each file holds; ``main`` prints
them):

* n = 1, 4: in the index block itself (elements 0-3), no other block;
* n = 5, 40: also in data blocks addressed from the index block (six of
  them: 16, 32, 32, 32, 64 and 64 elements -- elements 4-243); 5 needs the
  first (1 EADB), 40 the second as well (2 EADB), neither a super block;
* n = 3000: also in data blocks addressed from super blocks (element 244
  on): 4 EASB -- 4 x 64, 4 x 128, 8 x 128 and 8 x 256 elements, of the
  last of which four data blocks exist -- hence 6 + 4 + 4 + 8 + 4 = 26 EADB.

Data blocks stay unpaged up to 1024 elements each, that is for the first
131060 chunks of a dataset (checked: 131060 one-record chunks read, 131061
raise); paged ones are not read.

``sideways`` (4, 7) grows along its SECOND axis in chunks of (2, 1): the
array then runs along that axis first (libhdf5 "swizzles" the chunk
coordinates).  ``two_axes`` has two unlimited axes: a version-2 B-tree
index, which the reader refuses by name.

``record_input.nc``: the input of tests/test_gpu_record_dims.py laid out as
netCDF-4 does (dimension scales, ``_Netcdf4Dimid``, ``DIMENSION_LIST``
through ``attach_scale``), ``Time`` unlimited, every variable gzip 4 +
shuffle: a (Time=3, lat=6, lon=12) float64 field with NaNs stored as its
``_FillValue``, a (Time,) int32 counter and an ``xtime``-like char array.
``record_field`` below is the formula the test uses too.
"""
import os

import h5py
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'hdf5')
COUNTS = (1, 4, 5, 40, 3000)
FILL = 9.969209968386869e+36
PURE = 'This is a netCDF dimension but not a netCDF variable.'
rng = np.random.default_rng(11)
expected = {}


def record_field():
    """(3, 6, 12) float64; NaN where (t + i + j) % 7 == 0 and, in the
    second record, over the south-western 60 x 120 degrees."""
    t, i, j = np.meshgrid(np.arange(3.0), np.arange(6.0), np.arange(12.0),
                          indexing='ij')
    field = np.sin(0.5 * i) * np.cos(0.25 * j) + 0.125 * t
    field[(t + i + j) % 7 == 0] = np.nan
    field[1, :2, :4] = np.nan          # whole destination cells go missing
    return field


def records():
    path = os.path.join(OUT, 'records.h5')
    with h5py.File(path, 'w', libver='latest') as f:
        for n in COUNTS:
            f.create_dataset(f'plain_{n}', data=rng.standard_normal((n, 3)),
                             chunks=(1, 3), maxshape=(None, 3))
            f.create_dataset(f'packed_{n}',
                             data=rng.integers(-99, 99, (n, 4)).astype('f4'),
                             chunks=(1, 4), maxshape=(None, 4),
                             compression='gzip', compression_opts=4,
                             shuffle=True)
        f.create_dataset('sideways',
                         data=np.arange(28, dtype='i4').reshape(4, 7),
                         chunks=(2, 1), maxshape=(4, None))
        f.create_dataset('two_axes', data=np.arange(6.0).reshape(2, 3),
                         chunks=(1, 3), maxshape=(None, None))
    with h5py.File(path, 'r') as f:
        for name, d in f.items():
            expected[f'records:{name}'] = d[()]
    return path


def record_input():
    path = os.path.join(OUT, 'record_input.nc')
    field = record_field()
    stored = np.where(np.isnan(field), FILL, field)
    xtime = np.frombuffer(b'0001-01-010001-02-010001-03-01',
                          dtype='S1').reshape(3, 10)
    kw = dict(compression='gzip', compression_opts=4, shuffle=True)
    with h5py.File(path, 'w', libver='latest') as f:
        scales = {}
        for i, (name, size, unlimited) in enumerate(
                (('Time', 3, True), ('lat', 6, False), ('lon', 12, False),
                 ('StrLen', 10, False))):
            d = f.create_dataset(name, shape=(size,), dtype='<f4',
                                 chunks=(1,) if unlimited else None,
                                 maxshape=(None,) if unlimited else None)
            d.make_scale(f'{PURE}{size:10d}')
            d.attrs['_Netcdf4Dimid'] = np.int32(i)
            scales[name] = d
        for name, data, dims, chunks in (
                ('field', stored, ('Time', 'lat', 'lon'), (1, 6, 12)),
                ('count', np.array([10, 20, 30], 'i4'), ('Time',), (1,)),
                ('xtime', xtime, ('Time', 'StrLen'), (1, 10))):
            v = f.create_dataset(name, data=data, chunks=chunks,
                                 maxshape=(None,) + data.shape[1:], **kw)
            for axis, dim in enumerate(dims):
                v.dims[axis].attach_scale(scales[dim])
        f['field'].attrs['_FillValue'] = np.array([FILL])
        f['field'].attrs['units'] = np.bytes_('K')
        f.attrs['title'] = np.bytes_('record fixture')
    expected['record_input:field'] = field
    return path


def blocks(path):
    """How many blocks of each kind of the extensible arrays a file holds
    (every block starts with its four-byte signature)."""
    raw = open(path, 'rb').read()
    return {sig.decode(): raw.count(sig)
            for sig in (b'EAHD', b'EAIB', b'EADB', b'EASB')}


def main():
    os.makedirs(OUT, exist_ok=True)
    records()
    record_input()
    np.savez_compressed(os.path.join(OUT, 'expected_records.npz'),
                        **expected)
    # one dataset per file: which blocks does n records need?
    for n in COUNTS:
        tmp = os.path.join(OUT, '_probe.h5')
        with h5py.File(tmp, 'w', libver='latest') as f:
            f.create_dataset('x', data=np.zeros((n, 3)), chunks=(1, 3),
                             maxshape=(None, 3))
        print(n, 'records:', blocks(tmp))
        os.remove(tmp)
    for name in ('records.h5', 'record_input.nc', 'expected_records.npz'):
        print(name, os.path.getsize(os.path.join(OUT, name)))


if __name__ == '__main__':
    main()
