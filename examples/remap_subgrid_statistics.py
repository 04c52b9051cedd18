#!/usr/bin/env python
"""
Sub-grid statistics of a rough bottom depth through a conservative map (CDO's
``remapmin``, ``remapmax``, ``remapstd``, ``remapmedian``).  A remapped field
gives every destination cell the mean over the cell; coarse-graining also
wants to know what that mean hides: the shallowest and deepest depth under
the cell, the roughness (E3SM's ``SGH`` is the standard deviation of a fine
topography under each model cell), a median that a seamount does not pull.
With ``Remapper.statistics = {'bottomDepth': ['min', 'max', 'std',
'median']}`` the output of ``remap_numpy`` gains ``bottomDepth_min`` ... from
the rows of the ``conserve`` map that is there already.

The depth here is synthetic: a smooth basin shape on an MPAS mesh, rough
noise on top and a few seamounts.  The script prints the mean beside min,
max, std and median, how many cells have a mean outside ``[min, max]`` (none:
a mean of values with non-negative weights lies between them; one part in
1e12 is allowed for the rounding of the mean's sums) and how far mean and
median differ.

    python examples/remap_subgrid_statistics.py \\
        --mesh tests/golden/ref_fixtures/mpasMesh.nc --mesh-name oQU240 \\
        --res 4.0 [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pyremap_amd import (DataArray, Dataset, Remapper,  # noqa: E402
                         get_lat_lon_descriptor)
from pyremap_amd.io.netcdf import open_dataset  # noqa: E402

STATS = ['min', 'max', 'std', 'median']


def rough_depth(lat, lon, seed=1):
    """A bottom depth in m: a basin shape, rough noise, a few seamounts."""
    rng = np.random.default_rng(seed)
    depth = 3500.0 + 1200.0 * np.sin(3.0 * lat) * np.cos(2.0 * lon)
    depth = depth + 400.0 * rng.standard_normal(lat.shape)
    mounts = rng.random(lat.shape) < 0.02
    depth[mounts] = depth[mounts] * 0.15
    return np.maximum(depth, 10.0)


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', required=True, help='MPAS mesh file')
    parser.add_argument('--mesh-name', required=True)
    parser.add_argument('--res', type=float, default=4.0,
                        help='resolution of the lat-lon grid in degrees')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    cells = open_dataset(mesh)
    lat = np.asarray(cells['latCell'].values)
    lon = np.asarray(cells['lonCell'].values)
    ds = Dataset({'bottomDepth': DataArray(
        rough_depth(lat, lon), dims=('nCells',), attrs={'units': 'm'})})
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
        remapper.statistics = {'bottomDepth': STATS}
        out = remapper.remap_numpy(ds, 0.0)
    finally:
        os.chdir(here)
    mean = np.asarray(out['bottomDepth'].values, dtype=np.float64)
    stat = {name: np.asarray(out[f'bottomDepth_{name}'].values)
            for name in STATS}
    covered = ~np.isnan(stat['min'])
    assert np.array_equal(covered, ~np.isnan(mean))
    m = mean[covered]
    slack = 1e-12 * np.abs(m)
    outside = (m < stat['min'][covered] - slack) | \
        (m > stat['max'][covered] + slack)
    gap = m - stat['median'][covered]
    results = {
        'cells': int(mean.size), 'covered': int(covered.sum()),
        'mean_outside_min_max': int(outside.sum()),
        'largest_mean_minus_median': float(np.abs(gap).max()),
        'mean_std': float(stat['std'][covered].mean()),
    }
    print(f'{results["cells"]} destination cells, {results["covered"]} of '
          f'them covered by the mesh; bottomDepth in m')
    print('   cell      mean       min       max       std    median')
    for at in np.flatnonzero(covered.reshape(-1))[::max(
            1, results['covered'] // 8)][:8]:
        row = [a.reshape(-1)[at] for a in
               (mean, stat['min'], stat['max'], stat['std'], stat['median'])]
        print(f'{at:7d} ' + ' '.join(f'{v:9.1f}' for v in row))
    print(f'cells whose mean lies outside [min, max]: '
          f'{results["mean_outside_min_max"]}')
    print(f'mean - median: largest {results["largest_mean_minus_median"]:.1f}'
          f' m, mean of |mean - median| {np.abs(gap).mean():.1f} m; mean '
          f'std {results["mean_std"]:.1f} m')
    if results['mean_outside_min_max']:
        raise SystemExit('a mean outside the range of its own values')
    return results


if __name__ == '__main__':
    main()
