"""
The conserve maps and the four overlap wrappers behind them
(engine.overlap_latlon / overlap_meshes / overlap_pieces / overlap_grids,
weights.conserve_*), pinned on QU240-sized inputs so that the Python layer
between make_weights and the C ABI can be rearranged without moving a byte:

* the bytes of ``row, col, S, frac_b, area_a, area_b, frac_a`` of twelve
  maps against the SHA-256 digests of tests/golden/overlap_digests.json
  (these paths are bitwise repeatable: test_two_calls_are_bitwise_identical
  in each GPU conserve test file);
* the whole text of ``remap_last_error()`` for the error bits of the four
  routes against tests/golden/overlap_messages.json, a valid call after
  every failing one;
* the ``timing`` contract of the four wrappers: the same bytes with and
  without it, and the keys and values the dict receives;
* argument errors of overlap_pieces, which the host rejects before any
  kernel runs, and a valid call after them.

The digests are recorded with

    python tests/test_gpu_overlap_pinned.py --record [--commit HASH] [--out F]

on an MI355X, at the commit whose bytes are to be kept; the file names that
commit and every array's dtype, shape and own digest.  Recording keeps the
entries a file already has and adds the missing ones, each with the commit it
was recorded at; the messages go to overlap_messages.json the same way.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))))

from test_conserve_mesh_cpu import FIXTURES, QU240

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

DIGESTS = os.path.join(os.path.dirname(FIXTURES), 'overlap_digests.json')
MESSAGES = os.path.join(os.path.dirname(FIXTURES), 'overlap_messages.json')
ARRAYS = ('row', 'col', 'S', 'frac_b', 'area_a', 'area_b', 'frac_a')


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs an MI355X')
    torch.cuda.set_device(0)


# ---------------------------------------------------------------------------
# the inputs: QU240 and the global 10 degree grid
# ---------------------------------------------------------------------------

def qu240():
    from pyremap_amd import MpasCellMeshDescriptor
    return MpasCellMeshDescriptor(QU240, mesh_name='oQU240')


def grid10():
    from pyremap_amd.descriptor import get_lat_lon_descriptor
    return get_lat_lon_descriptor(10.0, 10.0)


def grid10_2d():
    """The 10 degree grid given by 2-D centre and corner arrays."""
    from pyremap_amd import LatLon2DGridDescriptor
    grid = grid10()
    lat, lon = np.meshgrid(grid.lat, grid.lon, indexing='ij')
    lat_c, lon_c = np.meshgrid(grid.lat_corner, grid.lon_corner,
                               indexing='ij')
    return LatLon2DGridDescriptor.create(lat, lon, lat_corner=lat_c,
                                         lon_corner=lon_c)


def icos27():
    """An icosahedral mesh of QU240's size (7 292 cells), from its file."""
    import tempfile
    from pyremap_amd import MpasCellMeshDescriptor, synthetic
    if 'icos27' not in _FILES:
        _FILES['icos27'] = os.path.join(tempfile.mkdtemp(), 'icos27.nc')
        synthetic.write_icosahedral_mesh(_FILES['icos27'], 27)
    return MpasCellMeshDescriptor(_FILES['icos27'], mesh_name='icos27')


_FILES = {}


def arctic500_2d():
    """The 500 km Arctic grid of test_gpu_conserve_grid.py as a 2-D grid."""
    from test_gpu_conserve_grid import descriptor_of, polar
    return descriptor_of(polar(6000.0, 5000.0, 500.0))


def atlantic_north_down():
    """A regional 2 degree grid whose latitude axis descends (its corners
    are turned to stay counter-clockwise: grid_cell's other branch)."""
    from pyremap_amd import LatLonGridDescriptor
    return LatLonGridDescriptor.create(
        np.linspace(70.0, 10.0, 31), np.linspace(-60.0, 60.0, 61),
        mesh_name='atlantic_north_down', regional=True)


def _vertex_to_grid():
    from pyremap_amd import MpasVertexMeshDescriptor, weights
    # (1 067 of these cells are concave, test_gpu_conserve_pieces.oracle: the
    # side goes over in pieces with a real parent array)
    return weights.conserve_polygons(
        MpasVertexMeshDescriptor(QU240, mesh_name='oQU240_vertex'), grid10())


def _maps():
    from pyremap_amd import weights
    return {
        'mesh_latlon_mesh_to_grid': lambda: weights.conserve_mesh_latlon(
            qu240(), grid10(), mesh_is_src=True),
        'mesh_latlon_grid_to_mesh': lambda: weights.conserve_mesh_latlon(
            qu240(), grid10(), mesh_is_src=False),
        'mesh_mesh_onto_itself': lambda: weights.conserve_mesh_mesh(
            qu240(), qu240()),
        'grid_mesh_to_2d': lambda: weights.conserve_grid(qu240(), grid10_2d()),
        # (fewer source cells than destination cells: src_is_a = False)
        'grid_2d_to_mesh': lambda: weights.conserve_grid(grid10_2d(), qu240()),
        'polygons_vertex_to_grid': _vertex_to_grid,
        'polygons_expanded_1p5': lambda: weights.conserve_polygons(
            qu240(), grid10(), expand_factor=1.5),
        # two different meshes: both values of dst_is_b with distinct sides
        # (icos27 has more cells, so it is side a either way)
        'mesh_mesh_qu240_to_icos27': lambda: weights.conserve_mesh_mesh(
            qu240(), icos27()),
        'mesh_mesh_icos27_to_qu240': lambda: weights.conserve_mesh_mesh(
            icos27(), qu240()),
        # both sides 2-D grids: the walker and the index side are grids
        'grid_2d_to_2d_polar': lambda: weights.conserve_grid(
            grid10_2d(), arctic500_2d()),
        'mesh_latlon_mesh_to_grid_lat_down':
            lambda: weights.conserve_mesh_latlon(
                qu240(), atlantic_north_down(), mesh_is_src=True),
        'mesh_latlon_grid_lat_down_to_mesh':
            lambda: weights.conserve_mesh_latlon(
                qu240(), atlantic_north_down(), mesh_is_src=False),
    }


MAPS = ('mesh_latlon_mesh_to_grid', 'mesh_latlon_grid_to_mesh',
        'mesh_mesh_onto_itself', 'grid_mesh_to_2d', 'grid_2d_to_mesh',
        'polygons_vertex_to_grid', 'polygons_expanded_1p5',
        'mesh_mesh_qu240_to_icos27', 'mesh_mesh_icos27_to_qu240',
        'grid_2d_to_2d_polar', 'mesh_latlon_mesh_to_grid_lat_down',
        'mesh_latlon_grid_lat_down_to_mesh')


def describe(m):
    """The digest of a map: SHA-256 over the raw bytes of :data:`ARRAYS` in
    that order, each C-contiguous, and dtype, shape and digest per array."""
    whole = hashlib.sha256()
    arrays = {}
    for name in ARRAYS:
        a = np.ascontiguousarray(getattr(m, name))
        raw = a.tobytes()
        whole.update(raw)
        arrays[name] = {'dtype': str(a.dtype), 'shape': list(a.shape),
                        'sha256': hashlib.sha256(raw).hexdigest()}
    return {'sha256': whole.hexdigest(), 'arrays': arrays}


# ---------------------------------------------------------------------------
# 1. pinned bytes
# ---------------------------------------------------------------------------

@pytest.mark.parametrize('name', MAPS)
def test_map_bytes_are_the_recorded_ones(name):
    assert set(_maps()) == set(MAPS)
    with open(DIGESTS) as f:
        recorded = json.load(f)
    want = recorded['maps'][name]
    m = _maps()[name]()
    assert m.n_s > 500
    assert m.row.dtype == np.int32 and m.col.dtype == np.int32
    got = describe(m)
    changed = [
        f'{k}: {got["arrays"][k]["dtype"]}{got["arrays"][k]["shape"]}, '
        f'recorded {want["arrays"][k]["dtype"]}{want["arrays"][k]["shape"]}'
        for k in ARRAYS if got['arrays'][k] != want['arrays'][k]]
    assert not changed, (
        f'{name}: bytes differ from those recorded at commit '
        f'{want.get("commit", recorded["commit"])} in {"; ".join(changed)}')
    assert got['sha256'] == want['sha256'], name


# ---------------------------------------------------------------------------
# 2. the timing contract of the four wrappers
# ---------------------------------------------------------------------------

def _dev(arrays):
    return [x if x is None or isinstance(x, int) else
            torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays]


def _overlap_calls():
    """{name: call(flag, timing)} of the four wrappers on QU240 and the 10
    degree grid, QU240 the side that is clipped."""
    from pyremap_amd import engine, weights
    mesh = weights.mesh_polygons(qu240())
    lat_e, lon_e, slack = weights.latlon_corners(grid10())
    quads = weights.cell_polygons(grid10())
    corners = weights.grid_corners(grid10())
    mesh_d, quads_d = _dev(mesh), _dev(quads)
    axes_d, corners_d = _dev((lat_e, lon_e)), _dev(corners)
    whole_mesh = mesh_d + [None, len(mesh[1])]
    whole_quads = quads_d + [None, len(quads[1])]
    return {
        'latlon': lambda flag, timing: engine.overlap_latlon(
            *mesh_d, *axes_d, slack, dst_is_mesh=flag, timing=timing),
        'meshes': lambda flag, timing: engine.overlap_meshes(
            mesh_d, quads_d, dst_is_b=flag, timing=timing),
        'pieces': lambda flag, timing: engine.overlap_pieces(
            whole_mesh, whole_quads, dst_is_b=flag, timing=timing),
        'grids': lambda flag, timing: engine.overlap_grids(
            mesh_d, corners_d, dst_is_b=flag, timing=timing),
    }


@pytest.mark.parametrize('name', ['latlon', 'meshes', 'pieces', 'grids'])
def test_timing_changes_no_byte_and_fills_the_dict(name):
    from pyremap_amd import engine
    call = _overlap_calls()[name]
    keys = {'n_pairs', 'ms'}
    if name == 'pieces':
        keys |= set(engine.PIECES_PHASES)
    for flag in (True, False):
        plain = [x.cpu().numpy() for x in call(flag, None)]
        timing = {}
        timed = [x.cpu().numpy() for x in call(flag, timing)]
        assert len(plain) == len(timed) == 6 and len(plain[0]) > 500
        for x, y in zip(plain, timed):
            assert x.dtype == y.dtype and x.shape == y.shape
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
        print(name, flag, timing)
        assert set(timing) == keys
        assert all(v >= 0 for v in timing.values())
        assert type(timing['n_pairs']) is int
        assert timing['n_pairs'] >= len(timed[0])


# ---------------------------------------------------------------------------
# 3. argument errors of overlap_pieces (rejected on the host) and a valid
# call after them
# ---------------------------------------------------------------------------

def test_pieces_argument_errors_and_a_valid_call_after_them():
    from pyremap_amd import engine, weights
    mesh = weights.mesh_polygons(qu240())
    quads = weights.cell_polygons(grid10())
    n = len(mesh[1])
    whole_quads = _dev(quads) + [None, len(quads[1])]
    parent = np.arange(n, dtype=np.int32)
    short = _dev(mesh) + [torch.from_numpy(parent[:-1].copy()).cuda(), n]
    with pytest.raises(ValueError) as e:
        engine.overlap_pieces(short, whole_quads, True)
    assert str(e.value) == f'overlap_pieces: {n - 1} parents for {n} pieces'
    down = parent.copy()
    down[[5, 6]] = down[[6, 5]]
    falling = _dev(mesh) + [torch.from_numpy(down).cuda(), n]
    for sides in ((falling, whole_quads), (whole_quads, falling)):
        with pytest.raises(ValueError, match='decreases') as e:
            engine.overlap_pieces(*sides, True)
        said = engine.load_library().remap_last_error().decode('utf-8',
                                                                'replace')
        assert 'decreases' in said
        assert str(e.value) == f'remap_overlap_pieces: {said}'
    good = _dev(mesh) + [torch.from_numpy(parent).cuda(), n]
    out = engine.overlap_pieces(good, whole_quads, True)
    torch.cuda.synchronize()
    assert len(out[0]) > 500 and len(out[3]) == len(quads[1])
    assert len(out[4]) == n


# ---------------------------------------------------------------------------
# 4. pinned messages: the error bits of the four routes as text
# ---------------------------------------------------------------------------

def _said():
    from pyremap_amd import engine
    return engine.load_library().remap_last_error().decode('utf-8', 'replace')


def _raises(call, *args):
    """call(*args) must fail with an EngineError (its message is read from
    the library afterwards)."""
    from pyremap_amd import engine

    def run():
        with pytest.raises(engine.EngineError):
            call(*args)
    return run


def _latlon_cases():
    import test_gpu_overlap_edges as edges
    from test_conserve_mesh_cpu import grid_arrays
    from test_gpu_conserve_mesh import gpu_map
    grid15 = grid_arrays(edges._deg(-90, 90, 15), edges._deg(-180, 180, 15))
    wide = grid_arrays([-10.0, 10.0], [0.0, 120.0, 240.0], regional=True)
    cases = {name: _raises(gpu_map, *bad[:4], *grid15, True)
             for name, bad in edges._bad_meshes().items()}
    cases['hemisphere'] = _raises(gpu_map, *edges._icos(4), *wide, True)
    cases['hemisphere_to_grid'] = _raises(gpu_map, *edges._icos(4), *wide,
                                          False)
    # (the test itself expects the failure; the message stays behind)
    cases['stale_minus_1'] = lambda: edges.test_stale_pair_count_raises(-1)
    cases['stale_plus_1'] = lambda: edges.test_stale_pair_count_raises(1)
    return (lambda: gpu_map(*edges._icos(4), *grid15, True)), cases


def _meshes_cases():
    from test_conserve_mesh_cpu import disc_mesh
    from test_conserve_meshes_cpu import icos_arrays
    from test_gpu_conserve_meshes import _copy, gpu_overlaps
    good = icos_arrays(6)
    voc, noc, lat_v, lon_v = _copy(good)
    noc[3] = voc.shape[1] + 1
    too_many = (voc, noc, lat_v, lon_v)
    voc, noc, lat_v, lon_v = _copy(good)
    voc[5, 1] = len(lat_v) + 7
    bad_index = (voc, noc, lat_v, lon_v)
    voc, noc, lat, lon = disc_mesh(np.radians(20.0), np.radians(30.0),
                                   np.radians(8.0))
    lat, lon = lat.copy(), lon.copy()
    lat[0] = 0.25 * lat[0] + 0.75 * np.radians(20.0)
    lon[0] = 0.25 * lon[0] + 0.75 * np.radians(30.0)
    dart = (voc, noc, lat, lon)
    cases = {}
    for name, bad in (('too_many', too_many), ('wide', _copy(good, width=11)),
                      ('bad_index', bad_index)):
        cases[name + '_a'] = _raises(gpu_overlaps, bad, good, True)
        cases[name + '_b'] = _raises(gpu_overlaps, good, bad, True)
    cases['dart_clips_to_b'] = _raises(gpu_overlaps, good, dart, True)
    cases['dart_clips_to_a'] = _raises(gpu_overlaps, good, dart, False)
    return (lambda: gpu_overlaps(good, icos_arrays(4), True)), cases


def _grids_cases():
    from test_conserve_meshes_cpu import icos_arrays
    from test_gpu_conserve_grid import gpu_overlaps, polar, radians
    mesh = icos_arrays(12)
    lat, lon = radians(polar(3000.0, 2000.0, 100.0))
    blat, blon = lat.copy(), lon.copy()
    for a in (blat, blon):
        a[5, 7], a[5, 8] = a[5, 8].copy(), a[5, 7].copy()
    vlat, vlon = lat.copy(), lon.copy()
    vlat[3, 4], vlon[3, 4] = vlat[3, 5], vlon[3, 5]
    vlat[4, 4], vlon[4, 4] = vlat[4, 5], vlon[4, 5]
    cases = {
        'bow_tie_b': _raises(gpu_overlaps, mesh, (blat, blon), True),
        'collapsed_b': _raises(gpu_overlaps, mesh, (vlat, vlon), True),
        'collapsed_a': _raises(gpu_overlaps, (vlat, vlon), mesh, True),
        'no_grid': _raises(gpu_overlaps, mesh, mesh, True),
    }
    return (lambda: gpu_overlaps(mesh, (lat, lon), True)), cases


def _pieces_cases():
    from test_conserve_meshes_cpu import icos_arrays
    from test_gpu_conserve_pieces import _ell, gpu_pieces, whole
    good, ell = icos_arrays(4), _ell()
    cases = {
        'ell_clips_to_b': _raises(gpu_pieces, whole(good), whole(ell), True),
        'ell_clips_to_a': _raises(gpu_pieces, whole(good), whole(ell), False),
    }
    return (lambda: gpu_pieces(whole(good), whole(icos_arrays(3)), True)), \
        cases


ROUTES = {'latlon': _latlon_cases, 'meshes': _meshes_cases,
          'grids': _grids_cases, 'pieces': _pieces_cases}


def messages_of(route):
    """{case: the library's message} of one route's failing calls, a valid
    call after each: its bytes are those of the call before any failure."""
    valid, cases = ROUTES[route]()
    first = valid()
    assert len(first[0]) > 100
    out = {}
    for name, call in cases.items():
        call()
        out[name] = _said()
        again = valid()
        for x, y in zip(first, again):
            assert x.dtype == y.dtype and x.shape == y.shape, name
            assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), name
    return out


@pytest.mark.parametrize('route', list(ROUTES))
def test_messages_are_the_recorded_ones(route):
    with open(MESSAGES) as f:
        want = json.load(f)['messages'][route]
    got = messages_of(route)
    for name in got:
        print(f'{route} {name}: {got[name]!r}')
    assert got == want


# ---------------------------------------------------------------------------
# recording
# ---------------------------------------------------------------------------

def record(argv):
    import argparse
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument('--record', action='store_true', required=True)
    ap.add_argument('--commit', default=None,
                    help='the commit the bytes are recorded at (default: '
                         'git rev-parse HEAD)')
    ap.add_argument('--out', default=DIGESTS)
    ap.add_argument('--messages', default=MESSAGES)
    args = ap.parse_args(argv)
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', 'HEAD'],
        cwd=os.path.dirname(os.path.abspath(__file__)), text=True).strip()
    assert torch.cuda.is_available(), 'recording needs an MI355X'
    torch.cuda.set_device(0)
    out = {'commit': commit, 'order': list(ARRAYS), 'maps': {}}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    assert out['order'] == list(ARRAYS)
    maps = _maps()
    added = [name for name in MAPS if name not in out['maps']]
    for name in added:
        out['maps'][name] = describe(maps[name]())
        if commit != out['commit']:
            out['maps'][name] = {'commit': commit, **out['maps'][name]}
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(f'recorded {added} at {commit} in {args.out}')
    said = {'commit': commit, 'messages': {}}
    if os.path.exists(args.messages):
        with open(args.messages) as f:
            said = json.load(f)
    for route in ROUTES:
        have = said['messages'].setdefault(route, {})
        for name, text in messages_of(route).items():
            have.setdefault(name, text)
    with open(args.messages, 'w') as f:
        json.dump(said, f, indent=1)
        f.write('\n')
    print(f'messages at {said["commit"]} in {args.messages}')


if __name__ == '__main__':
    record(sys.argv[1:])
