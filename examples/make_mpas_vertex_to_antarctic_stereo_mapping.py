#!/usr/bin/env python
"""
A first-order conservative (``conserve``, ESMF's ``aave``) mapping file from
the VERTICES of an MPAS mesh to an Antarctic polar stereographic grid without
ESMF (``map_tool='analytic'``), then a field on vertices remapped with
``remap_numpy``.

The cell around a vertex runs through the midpoints of its three edges and
the centres of its three cells.  Beside the coast a cell or an edge is
missing and the vertex itself takes its place: with one cell left the cell is
a kite, with two it is a hexagon with a reflex corner at the vertex --
concave.  Those are handed to the GPU as triangles and their overlaps added
up per cell (``pyremap_amd.weights.conserve_polygons``); the projection grid
takes part through its projected corners.

    python examples/make_mpas_vertex_to_antarctic_stereo_mapping.py \
        [--mesh tests/golden/ref_fixtures/mpasMesh.nc] [--mesh-name oQU240] \
        [--size 6000 5000] [--res 250] [-o OUT_DIR]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pyremap_amd import (DataArray, MpasVertexMeshDescriptor,  # noqa: E402
                         Remapper)
from pyremap_amd.io.netcdf import open_dataset  # noqa: E402
from pyremap_amd.polar import get_polar_descriptor  # noqa: E402

FIXTURES = os.path.join(ROOT, 'tests', 'golden', 'ref_fixtures')


def main(argv=None):
    parser = argparse.ArgumentParser(
        description=__doc__, formatter_class=argparse.RawTextHelpFormatter)
    parser.add_argument('--mesh', default=os.path.join(FIXTURES,
                                                       'mpasMesh.nc'))
    parser.add_argument('--mesh-name', default='oQU240')
    parser.add_argument('--size', type=float, nargs=2, default=(6000., 5000.),
                        metavar=('LX', 'LY'), help='extent of the grid, km')
    parser.add_argument('--res', type=float, default=250.0,
                        help='cell size, km')
    parser.add_argument('-o', dest='out_dir', default='.')
    args = parser.parse_args(argv)

    mesh = os.path.abspath(args.mesh)
    os.makedirs(args.out_dir, exist_ok=True)
    here = os.getcwd()
    os.chdir(args.out_dir)
    try:
        remapper = Remapper(
            ntasks=1, method='conserve', map_tool='analytic', use_tmp=False,
            src_descriptor=MpasVertexMeshDescriptor(
                mesh, mesh_name=f'{args.mesh_name}_vertices'),
            dst_descriptor=get_polar_descriptor(
                args.size[0], args.size[1], args.res, args.res,
                projection='antarctic'))
        # the map file lands under the default name
        # (map_<src>_to_<dst>_analyticaave.nc)
        remapper.build_map()
        # a field on vertices: the sine of their latitude
        field = DataArray(np.sin(np.asarray(
            open_dataset(mesh)['latVertex'].values)), dims=('nVertices',))
        out = remapper.remap_numpy(field, renormalization_threshold=0.01)
        values = np.asarray(out.values)
        print(f'{remapper.map_filename}: {args.mesh_name} vertices -> '
              f'{remapper.dst_descriptor.mesh_name} (conserve); '
              f'sin(latVertex) {values.shape}, '
              f'{np.isfinite(values).sum()} values, '
              f'{np.nanmin(values):.4f} .. {np.nanmax(values):.4f}')
    finally:
        os.chdir(here)
    return remapper


if __name__ == '__main__':
    main()
