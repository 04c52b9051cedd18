#!/usr/bin/env python
"""
Region ids through a conservative map, by largest area fraction (CDO's
``remaplaf``).  A field of labels -- region and basin ids, land-cover classes,
0/1/2 flags -- must not be averaged: the mean of region 3 and region 7 is
region 5.  With ``Remapper.categorical = ['regionId']`` every destination
cell takes the label whose overlap weights in its row of the map add up to
the most, so only labels the input holds come out, and the map is the
``conserve`` map that is there already.

The labels here are synthetic: int32 region ids on an MPAS mesh by latitude
band and longitude sector.  The script remaps them three ways -- through the
``conserve`` map with ``categorical``, through the same map as a plain mean,
and through a ``neareststod`` map -- and prints, for each, how many output
values are labels the input does not hold, and how many cells differ between
largest area fraction and nearest neighbour (one source point wins there even
if its cell covers a sliver of the destination cell).

    python examples/remap_region_ids.py \\
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \\
        --res 4.0 [--band 30] [--sector 60] [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import (DataArray, Dataset, Remapper,  # noqa: E402
                         get_lat_lon_descriptor)
from pyremap_amd.io.netcdf import open_dataset  # noqa: E402


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=4.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('--band', type=float, default=30.0,
                        help='height of a latitude band in degrees')
    parser.add_argument('--sector', type=float, default=60.0,
                        help='width of a longitude sector in degrees')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    cells = open_dataset(mesh)
    lat = np.rad2deg(np.asarray(cells['latCell'].values))
    lon = np.rad2deg(np.asarray(cells['lonCell'].values)) % 360.0
    sectors = int(np.ceil(360.0 / args.sector))
    # ids 11, 12, ... 21, 22, ...: band * 10 + sector would do for up to 9
    # sectors; any injective numbering does
    region = (np.floor((lat + 90.0) / args.band).astype(np.int32) *
              (sectors + 1) + np.floor(lon / args.sector).astype(np.int32) +
              1).astype(np.int32)
    held = set(region.tolist())
    ds = Dataset({'regionId': DataArray(region, dims=('nCells',))})
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        maps = {}
        for method in ('conserve', 'neareststod'):
            remapper = Remapper(ntasks=1, method=method, map_tool='analytic',
                                use_tmp=False)
            remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name)
            remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                             dlat=args.res)
            remapper.build_map()
            maps[method] = remapper
        mean = np.asarray(
            maps['conserve'].remap_numpy(ds, 0.0)['regionId'].values)
        maps['conserve'].categorical = ['regionId']
        out = maps['conserve'].remap_numpy(ds, 0.0)['regionId']
        fill = out.attrs['_FillValue']
        laf = np.asarray(out.values)
        nearest = np.asarray(
            maps['neareststod'].remap_numpy(ds, None)['regionId'].values)
    finally:
        os.chdir(here)
    assert laf.dtype == np.int32
    covered = laf != fill

    ids = np.array(sorted(held), dtype=np.float64)

    def invented(values):
        """Values further than 1e-6 from every region id of the input (the
        rounding of a mean of equal ids is not held against it)."""
        v = np.asarray(values, dtype=np.float64).reshape(-1, 1)
        return int((np.abs(v - ids[None, :]).min(axis=1) > 1e-6).sum())
    results = {
        'cells': int(laf.size), 'covered': int(covered.sum()),
        'laf_invented': invented(laf[covered]),
        'mean_invented': invented(mean[covered]),
        'nearest_invented': invented(nearest[covered]),
        'laf_differs_from_nearest': int((laf != nearest)[covered].sum()),
    }
    print(f'{results["cells"]} destination cells, {results["covered"]} of '
          f'them covered by the mesh; {len(held)} region ids')
    print('values that are no region id of the input (by more than 1e-6):')
    print(f'  conserve, categorical (largest area fraction) '
          f'{results["laf_invented"]:6d}')
    print(f'  conserve, plain mean                          '
          f'{results["mean_invented"]:6d}')
    print(f'  neareststod                                   '
          f'{results["nearest_invented"]:6d}')
    print(f'cells where largest area fraction and nearest neighbour differ: '
          f'{results["laf_differs_from_nearest"]}')
    if results['laf_invented'] or results['nearest_invented']:
        raise SystemExit('a label the input does not hold came out')
    return results


if __name__ == '__main__':
    main()
