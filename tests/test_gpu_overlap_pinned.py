"""
The conserve maps and the four overlap wrappers behind them
(engine.overlap_latlon / overlap_meshes / overlap_pieces / overlap_grids,
weights.conserve_*), pinned on QU240-sized inputs so that the Python layer
between make_weights and the C ABI can be rearranged without moving a byte:

* the bytes of ``row, col, S, frac_b, area_a, area_b, frac_a`` of seven maps
  against the SHA-256 digests of tests/golden/overlap_digests.json (these
  paths are bitwise repeatable: test_two_calls_are_bitwise_identical in each
  GPU conserve test file);
* the ``timing`` contract of the four wrappers: the same bytes with and
  without it, and the keys and values the dict receives;
* argument errors of overlap_pieces, which the host rejects before any
  kernel runs, and a valid call after them.

The digests are recorded with

    python tests/test_gpu_overlap_pinned.py --record [--commit HASH] [--out F]

on an MI355X, at the commit whose bytes are to be kept; the file names that
commit and every array's dtype, shape and own digest.
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
    }


MAPS = ('mesh_latlon_mesh_to_grid', 'mesh_latlon_grid_to_mesh',
        'mesh_mesh_onto_itself', 'grid_mesh_to_2d', 'grid_2d_to_mesh',
        'polygons_vertex_to_grid', 'polygons_expanded_1p5')


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
        f'{recorded["commit"]} in {"; ".join(changed)}')
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
    args = ap.parse_args(argv)
    commit = args.commit or subprocess.check_output(
        ['git', 'rev-parse', 'HEAD'],
        cwd=os.path.dirname(os.path.abspath(__file__)), text=True).strip()
    assert torch.cuda.is_available(), 'recording needs an MI355X'
    torch.cuda.set_device(0)
    maps = _maps()
    out = {'commit': commit, 'order': list(ARRAYS),
           'maps': {name: describe(maps[name]()) for name in MAPS}}
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    print(f'recorded {len(MAPS)} maps at {commit} in {args.out}')


if __name__ == '__main__':
    record(sys.argv[1:])
