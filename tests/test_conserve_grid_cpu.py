"""
Weights to and from a grid given by 2-D latitude / longitude arrays
(LatLon2DGridDescriptor), the parts that run without a GPU: explicit corner
arrays on the descriptor, bilinear / neareststod towards the grid's cell
centres, and the dispatch of ``conserve`` (the served pairs go to the GPU,
everything else and every malformed corner array is a ValueError).
"""
import numpy as np
import pytest

from test_conserve_mesh_cpu import QU240


def arctic(lx=6000.0, ly=5000.0, d=500.0, **kwargs):
    """An Arctic stereographic grid as a 2-D grid with projected corners."""
    from pyremap_amd import LatLon2DGridDescriptor
    from pyremap_amd.polar import get_polar_descriptor
    p = get_polar_descriptor(lx, ly, d, d, projection='arctic')
    lat_c, lon_c = p.project_to_lat_lon(*np.meshgrid(p.x_corner, p.y_corner))
    lat, lon = p.project_to_lat_lon(*np.meshgrid(p.x, p.y))
    return LatLon2DGridDescriptor.create(lat, lon, lat_corner=lat_c,
                                         lon_corner=lon_c, **kwargs)


def test_create_keeps_explicit_corners():
    from pyremap_amd import LatLon2DGridDescriptor
    from pyremap_amd.descriptor.corners import extrapolate_corners_2d
    d = arctic()
    assert d.lat.shape == (11, 13) and d.lat_corner.shape == (12, 14)
    # the pole is a corner-row's neighbour, the seam is crossed: nothing an
    # extrapolation in lat-lon space would give
    assert d.lon_corner.min() < -170.0 and d.lon_corner.max() > 170.0
    assert not np.allclose(d.lon_corner, extrapolate_corners_2d(d.lon))
    again = LatLon2DGridDescriptor.create(d.lat, d.lon,
                                          lat_corner=d.lat_corner.tolist(),
                                          lon_corner=d.lon_corner.tolist())
    assert np.array_equal(again.lat_corner, d.lat_corner)
    assert np.array_equal(again.lon_corner, d.lon_corner)
    assert again.dims == ['y', 'x'] and tuple(again.dim_sizes) == (11, 13)
    # without the keywords: the extrapolated corners, as before
    lat, lon = np.meshgrid(np.arange(10.0, 40.0, 2.0),
                           np.arange(100.0, 130.0, 3.0), indexing='ij')
    plain = LatLon2DGridDescriptor.create(lat, lon)
    assert np.array_equal(plain.lat_corner, extrapolate_corners_2d(lat))
    assert np.array_equal(plain.lon_corner, extrapolate_corners_2d(lon))
    assert np.allclose(plain.lat_corner[:, 0], np.arange(9.0, 40.0, 2.0))
    with pytest.raises(ValueError, match=r'expected \(ny \+ 1, nx \+ 1\)'):
        LatLon2DGridDescriptor.create(lat, lon, lat_corner=lat,
                                      lon_corner=lon)
    with pytest.raises(ValueError, match='go together'):
        LatLon2DGridDescriptor.create(lat, lon, lat_corner=plain.lat_corner)


@pytest.mark.parametrize('method', ['bilinear', 'neareststod'])
def test_latlon_towards_a_2d_grid_takes_its_centres(method):
    from pyremap_amd import PointCollectionDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    src = get_lat_lon_descriptor(5.0, 5.0)
    grid = arctic()
    got = build_weights(src, grid, method)
    pts = PointCollectionDescriptor(grid.lat.reshape(-1),
                                    grid.lon.reshape(-1), 'centres')
    want = build_weights(src, pts, method)
    assert list(got.dst_grid_dims) == [13, 11]
    assert got.n_a == want.n_a and got.n_b == want.n_b == 143
    assert len(got.S) > 100
    for name in ('row', 'col', 'S', 'frac_b'):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


def test_mesh_towards_a_2d_grid_takes_its_centres():
    from pyremap_amd import MpasCellMeshDescriptor, PointCollectionDescriptor
    from pyremap_amd.weights import build_weights
    src = MpasCellMeshDescriptor(QU240, mesh_name='oQU240')
    grid = arctic(units='degrees')
    got = build_weights(src, grid, 'bilinear')
    pts = PointCollectionDescriptor(grid.lat.reshape(-1),
                                    grid.lon.reshape(-1), 'centres')
    want = build_weights(src, pts, 'bilinear')
    assert list(got.dst_grid_dims) == [13, 11]
    assert len(got.S) > 100
    for name in ('row', 'col', 'S', 'frac_b'):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name


def test_from_a_2d_grid_only_conserve_is_served():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights
    for method in ('bilinear', 'neareststod'):
        with pytest.raises(TypeError, match='analytic weights need a '
                                            'LatLonGridDescriptor'):
            build_weights(arctic(), get_lat_lon_descriptor(5.0, 5.0), method)


def _served_pairs():
    from pyremap_amd import MpasCellMeshDescriptor
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    grid = arctic()
    others = (MpasCellMeshDescriptor(QU240, mesh_name='oQU240'),
              get_lat_lon_descriptor(10.0, 10.0),
              get_lat_lon_descriptor(5.0, 5.0, lon_min=0.0, lon_max=90.0,
                                     lat_min=40.0, lat_max=90.0),
              arctic(3000.0, 2000.0, 100.0))
    return [(grid, o) for o in others] + [(o, grid) for o in others]


def test_conserve_with_a_2d_grid_needs_the_gpu():
    import torch
    from pyremap_amd import engine
    from pyremap_amd.weights import build_weights, conserve_grid
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    for a, b in _served_pairs():
        with pytest.raises(engine.EngineError, match='no HIP device'):
            build_weights(a, b, 'conserve')
        with pytest.raises(engine.EngineError, match='no HIP device'):
            conserve_grid(a, b)


def test_unserved_conserve_pairs_name_the_served_ones():
    from pyremap_amd import (MpasCellMeshDescriptor, MpasEdgeMeshDescriptor,
                             MpasVertexMeshDescriptor,
                             PointCollectionDescriptor)
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.polar import get_polar_descriptor
    from pyremap_amd.weights import build_weights, conserve_grid
    grid = arctic()
    bare = MpasCellMeshDescriptor(mesh_name='m', lat=np.zeros(3),
                                  lon=np.arange(3.0))
    unserved = (PointCollectionDescriptor(np.zeros(4), np.arange(4.0), 'p'),
                MpasEdgeMeshDescriptor(QU240, mesh_name='m'),
                MpasVertexMeshDescriptor(QU240, mesh_name='m'),
                bare,
                get_polar_descriptor(6000.0, 5000.0, 500.0, 500.0))
    served = ('served between it and an MPAS cell mesh given by its mesh '
              'file, a LatLonGridDescriptor or another 2-D lat-lon grid')
    for other in unserved:
        for a, b in ((grid, other), (other, grid)):
            with pytest.raises(ValueError, match=served) as err:
                build_weights(a, b, 'conserve')
            assert type(other).__name__ in str(err.value)
    with pytest.raises(ValueError, match='without its mesh file'):
        build_weights(grid, bare, 'conserve')
    with pytest.raises(ValueError, match='neither side is one'):
        conserve_grid(get_lat_lon_descriptor(10.0, 10.0),
                      get_lat_lon_descriptor(5.0, 5.0))


def test_malformed_corner_arrays():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    from pyremap_amd.weights import build_weights, grid_corners
    latlon = get_lat_lon_descriptor(10.0, 10.0)
    good = arctic()
    lat, lon = grid_corners(good)
    assert lat.shape == (12, 14) and np.abs(lat).max() <= 0.5 * np.pi
    assert np.allclose(np.degrees(lat), good.lat_corner)

    def broken(change):
        d = arctic()
        change(d)
        return d

    def too_small(d):
        d.lat_corner = d.lat_corner[:-1]

    def not_finite(d):
        d.lon_corner[2, 3] = np.nan

    def infinite(d):
        d.lat_corner[0, 0] = np.inf

    def beyond(d):
        d.lat_corner[4, 4] = 90.5

    for change, match in ((too_small, r'\(ny \+ 1, nx \+ 1\) = \(12, 14\)'),
                          (not_finite, 'must be finite'),
                          (infinite, 'must be finite'),
                          (beyond, 'beyond \\+-90 degrees')):
        for a, b in ((broken(change), latlon), (latlon, broken(change))):
            with pytest.raises(ValueError, match=match):
                build_weights(a, b, 'conserve')
    # rounding past the pole is the pole
    d = arctic(units='radians')
    d.lat_corner = np.radians(good.lat_corner)
    d.lon_corner = np.radians(good.lon_corner)
    d.lat_corner[5, 5] = 0.5 * np.pi + 1e-12
    assert grid_corners(d)[0][5, 5] == 0.5 * np.pi
    # a lat-lon grid: the outer product of its corner axes, poles clipped
    lat, lon = grid_corners(latlon)
    assert lat.shape == lon.shape == (19, 37)
    assert lat[0, 0] == -0.5 * np.pi and lat[-1, 5] == 0.5 * np.pi
    assert np.all(lat[:, 1:] == lat[:, :1]) and np.all(lon[1:] == lon[:1])


def test_remapper_build_map_text_names_the_2d_grid():
    from pyremap_amd import Remapper
    with pytest.raises(NotImplementedError, match='2-D lat-lon grid'):
        Remapper(map_tool='esmf').build_map()
    assert 'LatLon2DGridDescriptor' in Remapper.build_map.__doc__


def test_the_library_exports_the_grid_calls():
    from pyremap_amd import engine
    assert 'remap_overlap_grids_sizes' in engine.EXPORTS
    assert 'remap_overlap_grids' in engine.EXPORTS
