"""
Conservative weights between two MPAS cell meshes, the parts that run
without a GPU: the numpy reference clipper of tests/test_conserve_mesh_cpu.py
applied mesh against mesh (it tiles the sphere), the dispatch of
build_weights (every error it raised before is still raised) and the engine
error without a device.

The mesh-against-mesh reference is the one tests/test_gpu_conserve_meshes.py
checks the GPU against.
"""
import numpy as np
import pytest

import test_conserve_mesh_cpu as base
from test_conserve_mesh_cpu import (QU240, mesh_cells_from_arrays,
                                    polygon_area, reference_overlaps)


def icos_arrays(n, land=None):
    """(verticesOnCell, nEdgesOnCell, latVertex, lonVertex) of the
    icosahedral mesh n."""
    from pyremap_amd import synthetic
    m = synthetic.icosahedral_mesh(n, land)
    return (m['verticesOnCell'], m['nEdgesOnCell'], m['latVertex'],
            m['lonVertex'])


def mesh_overlaps(arrays_a, arrays_b):
    """The numpy reference between two meshes given as arrays: (a, b, A)
    for every pair with a non-zero overlap, a's polygon clipped by b's,
    and both sets of polygon areas."""
    cells_a = mesh_cells_from_arrays(*arrays_a)
    cells_b = mesh_cells_from_arrays(*arrays_b)
    ref = reference_overlaps(cells_a, cells_b)
    area_a = np.array([polygon_area(p) for p in cells_a])
    area_b = np.array([polygon_area(p) for p in cells_b])
    return ref, area_a, area_b


def test_reference_meshes_tile_the_sphere():
    """Two icosahedral meshes that share no vertex: their overlaps add up
    to the sphere, and to every cell's own area on either side."""
    ref, area_a, area_b = mesh_overlaps(icos_arrays(4), icos_arrays(3))
    a, b, A = (np.array(x) for x in zip(*ref))
    assert abs(A.sum() - 4 * np.pi) < 1e-12
    assert abs(area_a.sum() - 4 * np.pi) < 1e-12
    assert abs(area_b.sum() - 4 * np.pi) < 1e-12
    per_a = np.bincount(a.astype(np.int64), weights=A, minlength=len(area_a))
    per_b = np.bincount(b.astype(np.int64), weights=A, minlength=len(area_b))
    assert np.abs(per_a / area_a - 1.0).max() < 1e-12
    assert np.abs(per_b / area_b - 1.0).max() < 1e-12
    # the same pairs the other way round (b clipped by a), the same areas
    back = {(j, i): s for i, j, s in
            reference_overlaps(mesh_cells_from_arrays(*icos_arrays(3)),
                               mesh_cells_from_arrays(*icos_arrays(4)))}
    big = {(i, j) for i, j, s in ref if s > 1e-14}
    assert big <= set(back)
    assert max(abs(back[(i, j)] - s) for i, j, s in ref if (i, j) in big) \
        < 1e-15


def test_reference_mesh_onto_itself():
    """A mesh clipped by itself: every cell whole on its own diagonal, the
    neighbours' shared edges leave nothing."""
    arrays = icos_arrays(3)
    ref, area_a, _ = mesh_overlaps(arrays, arrays)
    diag = {i: s for i, j, s in ref if i == j}
    assert sorted(diag) == list(range(len(area_a)))
    assert max(abs(diag[i] / area_a[i] - 1.0) for i in diag) < 1e-13
    off = sum(s for i, j, s in ref if i != j)
    assert off < 1e-14


def test_conserve_mesh_dispatch_keeps_every_existing_error(tmp_path):
    from pyremap_amd import (MpasCellMeshDescriptor, MpasEdgeMeshDescriptor,
                             MpasVertexMeshDescriptor, synthetic)
    from pyremap_amd.weights import build_weights
    base.test_conserve_dispatch_keeps_every_existing_error()
    path = str(tmp_path / 'icos4.nc')
    synthetic.write_icosahedral_mesh(path, 4)
    mesh = MpasCellMeshDescriptor(path)
    bare = MpasCellMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                  lon=np.arange(3.0))
    # a cell mesh without its file on either side: the old messages
    with pytest.raises(ValueError, match='only bilinear'):
        build_weights(bare, mesh, 'conserve')
    with pytest.raises(ValueError, match='only bilinear'):
        build_weights(mesh, bare, 'conserve')
    # edge and vertex meshes against a cell mesh
    for cls in (MpasEdgeMeshDescriptor, MpasVertexMeshDescriptor):
        with pytest.raises(ValueError, match='only bilinear'):
            build_weights(cls(QU240, mesh_name='m'), mesh, 'conserve')
        with pytest.raises(ValueError, match='only bilinear'):
            build_weights(mesh, cls(QU240, mesh_name='m'), 'conserve')


def test_conserve_between_mesh_files_needs_the_gpu(tmp_path):
    """MPAS cell mesh <-> MPAS cell mesh conserve goes to the GPU: without
    one it raises the engine's error, in both directions; no CPU path."""
    import torch
    from pyremap_amd import MpasCellMeshDescriptor, engine, synthetic
    from pyremap_amd.weights import build_weights
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    path = str(tmp_path / 'icos8.nc')
    synthetic.write_icosahedral_mesh(path, 8)
    qu240 = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    icos = MpasCellMeshDescriptor(path)
    for a, b in ((qu240, icos), (icos, qu240)):
        with pytest.raises(engine.EngineError, match='no HIP device'):
            build_weights(a, b, 'conserve')


def test_remapper_build_map_text_names_mesh_to_mesh():
    from pyremap_amd import Remapper
    with pytest.raises(NotImplementedError, match='or another MPAS cell '
                                                  'mesh'):
        Remapper(map_tool='esmf').build_map()


def test_engine_declares_the_mesh_entry_points():
    from pyremap_amd import engine
    assert 'remap_overlap_meshes_sizes' in engine.EXPORTS
    assert 'remap_overlap_meshes' in engine.EXPORTS
    names = [f[0] for f in engine._OverlapMesh._fields_]
    assert names == ['n_cells', 'n_vertices', 'max_edges', 'reserved',
                     'vertices_on_cell', 'n_edges_on_cell', 'lat_vertex',
                     'lon_vertex']
