#!/opt/conda/bin/python3.9
"""
Cross-check of the chunked / filtered NetCDF-4 files that
pyremap_amd/io/hdf5_write.py writes against libhdf5 (TEST INFRASTRUCTURE
ONLY; runs under an interpreter with h5py, started by
tests/test_hdf5_records_cpu.py in a subprocess):

    python tests/check_records_h5py.py file.nc expected.npz

``expected.npz``: ``var/<name>`` -> values, and ``__meta__``, a JSON string
with ``dimensions`` (name -> size, in order), ``unlimited`` (names),
``variables`` (name -> dimension names) and ``storage`` (name -> ``{chunks,
complevel, shuffle}``, ``chunks`` null for contiguous data).  Through h5py
the file must give: the values; ``maxshape`` with ``None`` exactly on the
unlimited axes; the chunk shape, ``compression == 'gzip'`` with its level
and the shuffle flag as asked; ``H5DSis_scale`` on every dimension scale,
the unallocated placeholder of an unlimited dimension included; every axis
of every variable resolving through ``dims[i]`` to its scale.
"""
import json
import sys

import h5py
import numpy as np


def main():
    path, expected = sys.argv[1], np.load(sys.argv[2], allow_pickle=False)
    meta = json.loads(str(expected['__meta__']))
    unlimited = set(meta['unlimited'])
    with h5py.File(path, 'r') as f:
        assert sorted(f.keys()) == sorted(set(meta['variables']) |
                                          set(meta['dimensions']))
        for dim, size in meta['dimensions'].items():
            d = f[dim]
            assert h5py.h5ds.is_scale(d.id), dim
            assert d.shape == (size,), (dim, d.shape)
            assert d.maxshape == ((None,) if dim in unlimited else (size,)), \
                (dim, d.maxshape)
            if dim in unlimited:
                assert d.chunks is not None, dim
            assert int(d.attrs['_Netcdf4Dimid']) == \
                list(meta['dimensions']).index(dim)
            if dim not in meta['variables']:
                # a placeholder: never allocated
                assert d.id.get_offset() is None
                assert d.id.get_storage_size() == 0, dim
        for name, dims in meta['variables'].items():
            d = f[name]
            want = expected[f'var/{name}']
            got = d[()]
            assert got.dtype == want.dtype, (name, got.dtype, want.dtype)
            np.testing.assert_array_equal(got, want, err_msg=name)
            # one record at a time as well: a look-up in the chunk B-tree
            # per read, not the iteration d[()] does
            if dims and dims[0] in unlimited:
                for i in sorted({0, len(want) // 2, len(want) - 1}
                                if len(want) else ()):
                    np.testing.assert_array_equal(d[i], want[i],
                                                  err_msg=f'{name}[{i}]')
            assert d.maxshape == tuple(
                None if dim in unlimited else n
                for dim, n in zip(dims, want.shape)), (name, d.maxshape)
            store = meta['storage'][name]
            chunks = None if store['chunks'] is None \
                else tuple(store['chunks'])
            assert d.chunks == chunks, (name, d.chunks, chunks)
            if store['complevel']:
                assert d.compression == 'gzip', (name, d.compression)
                assert d.compression_opts == store['complevel'], \
                    (name, d.compression_opts)
            else:
                assert d.compression is None, (name, d.compression)
            assert bool(d.shuffle) == bool(store['shuffle']), name
            if dims == [name]:
                continue                       # a scale lists no scale
            assert len(d.dims) == len(dims)
            for axis, dim in enumerate(dims):
                scales = [s.name.lstrip('/') for s in d.dims[axis].values()]
                assert scales == [dim], (name, axis, scales, dim)
    print(f'OK {path}: {len(meta["variables"])} variables, '
          f'{len(meta["dimensions"])} dimension scales through libhdf5')


if __name__ == '__main__':
    main()
