#!/usr/bin/env python
"""
Sub-grid composition through a conservative map: what share of every
destination cell each class, or each value range, takes.  Largest area
fraction (``Remapper.categorical``) keeps the dominant region id of a cell
and throws the mixture away; percent cover per land-cover type, elevation or
depth bands and fractional region masks need the mixture itself.  With
``Remapper.fractions = {'regionId': dict(classes=None), 'bottomDepth':
dict(bins=[...])}`` the output gains ``regionId_frac`` (one layer per region
id) and ``bottomDepth_frac`` (one layer per depth band: the hypsometry under
the cell), from the rows of the ``conserve`` map that is there already, one
launch per variable.

The fields here are synthetic: int32 region ids on an MPAS mesh by latitude
band and longitude sector, and a rough ``bottomDepth``.  The script prints
that the fractions of every covered cell sum to 1, how many cells hold more
than one region, and that the argmax over the classes is what ``categorical``
gives, counting the cells where a tie between two regions makes them differ
(largest area fraction keeps the region it met first in the row, the argmax
the one with the lower id).

    python examples/remap_class_fractions.py \\
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

EDGES = [0.0, 500.0, 1000.0, 2000.0, 3000.0, 4000.0, np.inf]


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
    region = (np.floor((lat + 90.0) / args.band).astype(np.int32) *
              (sectors + 1) + np.floor(lon / args.sector).astype(np.int32) +
              1).astype(np.int32)
    rng = np.random.default_rng(7)
    depth = np.clip(
        2600.0 + 2200.0 * np.sin(np.radians(3.0 * lon)) *
        np.cos(np.radians(2.0 * lat)) + 300.0 * rng.standard_normal(len(lat)),
        5.0, None)
    ds = Dataset({'regionId': DataArray(region, dims=('nCells',)),
                  'bottomDepth': DataArray(depth, dims=('nCells',),
                                           attrs={'units': 'm'})})
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        remapper = Remapper(ntasks=1, method='conserve', map_tool='analytic',
                            use_tmp=False)
        remapper.src_from_mpas(filename=mesh, mesh_name=args.mesh_name)
        remapper.dst_descriptor = get_lat_lon_descriptor(dlon=args.res,
                                                         dlat=args.res)
        remapper.build_map()
        remapper.categorical = ['regionId']
        remapper.fractions = {'regionId': dict(classes=None),
                              'bottomDepth': dict(bins=EDGES)}
        out = remapper.remap_numpy(ds, 0.0)
    finally:
        os.chdir(here)
    laf = np.asarray(out['regionId'].values)
    fill = out['regionId'].attrs['_FillValue']
    frac = np.asarray(out['regionId_frac'].values)          # (C, lat, lon)
    ids = np.asarray(out['regionId_class'].values)
    bands = np.asarray(out['bottomDepth_frac'].values)      # (bins, lat, lon)
    bnds = np.asarray(out['bottomDepth_bin_bnds'].values)
    covered = ~np.isnan(frac[0])
    assert np.array_equal(covered, laf != fill)
    assert np.array_equal(covered, ~np.isnan(bands[0]))

    top = np.sort(frac[:, covered], axis=0)
    tie = top[-1] == top[-2]
    argmax = ids[np.argmax(frac[:, covered], axis=0)]
    differs = argmax != laf[covered]
    results = {
        'cells': int(laf.size), 'covered': int(covered.sum()),
        'classes': int(len(ids)),
        'class_sum_error': float(np.abs(frac[:, covered].sum(axis=0)
                                        - 1.0).max()),
        'bin_sum_error': float(np.abs(bands[:, covered].sum(axis=0)
                                      - 1.0).max()),
        'mixed_cells': int((top[-1] < 1.0).sum()),
        'argmax_differs': int(differs.sum()),
        'argmax_differs_at_ties': int((differs & tie).sum()),
    }
    print(f'{results["cells"]} destination cells, {results["covered"]} of '
          f'them covered by the mesh; {results["classes"]} region ids, '
          f'{len(bnds)} depth bands')
    print(f'fractions of the region ids: sum to 1 within '
          f'{results["class_sum_error"]:.1e} on covered cells; '
          f'{results["mixed_cells"]} cells hold more than one region')
    print(f'fractions of the depth bands: sum to 1 within '
          f'{results["bin_sum_error"]:.1e} on covered cells')
    share = np.nanmean(bands[:, covered], axis=1)
    for (lo, hi), s in zip(bnds, share):
        print(f'  {lo:6.0f} m to {hi:6.0f} m: {100.0 * s:5.1f} % of a cell '
              f'on average')
    print(f'argmax over the classes against categorical (largest area '
          f'fraction): {results["argmax_differs"]} cells differ, '
          f'{results["argmax_differs_at_ties"]} of them at a tie')
    if results['argmax_differs'] != results['argmax_differs_at_ties']:
        raise SystemExit('the argmax of the fractions and the largest area '
                         'fraction differ away from a tie')
    return results


if __name__ == '__main__':
    main()
